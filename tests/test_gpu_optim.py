"""The optimiser kernels of customnerf_amd/csrc/misc.hip (k_adam, k_adam_scaled, k_adam_scaled_multi, k_scaler_check, k_scaler_update, k_dp_pack,
k_dp_reduce) against the plain restatement of tests/optim_restatement.py, which tests/test_optim_restatement_host.py pins to torch on the CPU.

The Adam kernels are float32, the restatement float64, so they differ by rounding.  How much is allowed is not a fixed number: float32
torch.optim.Adam, run on the same device over the same gradients, is measured against the restatement by the same three quantities
(max |dp| / lr; max |dv| / v_ref; max |dm| / a_ref, a_ref being m's recurrence driven by |g'|), and a kernel may deviate at most BOUND = 4 times
that, per quantity and checkpointed step.  (The kernel differs from torch's float32 by a float32 1/sqrt(bc2) it multiplies with where torch
divides, by a float32 lr/bc1 and by the order of the last multiply and divide: a few ulp per step each, none a modelling difference.)
torch's deviation is taken over all tensors of a case together: its maximum over the 1, 2 or 3 elements of the smallest tensors can be exactly
zero by luck, and four times zero is no bound.  Each kernel tensor is held to it on its own.

Measured on an MI355X (kernel / float32 torch, both against float64; the worst over all tensors; k_adam, k_adam_scaled and k_adam_scaled_multi
gave the same figures to the digits shown):
                                   max |dp| / lr          max |dv| / v_ref       max |dm| / a_ref
    scale 65536           step 1   2.18e-07 / 2.18e-07    1.08e-07 / 1.00e-07    5.67e-08 / 5.67e-08
                          step 5   7.80e-07 / 8.45e-07    2.19e-07 / 2.19e-07    1.58e-07 / 1.37e-07
                          step 300 3.35e-05 / 3.72e-05    8.10e-07 / 1.03e-06    1.52e-07 / 1.27e-07
    scale 3000, extra 1/3 step 1   2.18e-07 / 2.24e-07    1.88e-07 / 1.86e-07    9.50e-08 / 9.50e-08
                          step 5   9.81e-07 / 8.40e-07    2.76e-07 / 2.53e-07    1.81e-07 / 1.99e-07
                          step 300 4.08e-05 / 3.95e-05    9.52e-07 / 9.52e-07    1.69e-07 / 1.47e-07
    second pass, n = 4 195 333     8.43e-07 / 7.78e-07    1.64e-07 / 1.19e-07    1.15e-07 / 1.06e-07      (k_adam, k_adam_scaled)
    second pass, n = 65 537        7.76e-07 / 6.87e-07    1.42e-07 / 1.09e-07    1.04e-07 / 9.98e-08      (k_adam_scaled_multi)
    step k + 1, every k            equal (ratio 1.00)     1.15e-07 / 8.46e-08    9.04e-08 / 6.73e-08
The largest ratio is 1.38, against the 4 allowed.

Two things these tests found are fixed with them: cn_scaler_update grew the scale 2^127 to inf (torch keeps the scale when the grown one is
not finite), and the tail loop of k_dp_pack lost the sign of a -0 product and rounded once where its vector body rounds twice.
"""
import ctypes

import numpy as np
import pytest
import torch

import optim_restatement as orr

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.99), 1e-15
BOUND = 4.0
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099]
LRS = [1e-2, 5e-3, 2e-3, 1e-3, 7e-4, 5e-4, 3e-4, 2e-2, 1e-4, 5e-3]          # one per size: the multi-tensor launch carries a learning rate per job
LONG_N, CHECKPOINTS = 4099, (1, 5, 300)
SCALES = {"pow2": (65536.0, 1.0), "odd": (3000.0, 1.0 / 3.0)}                # (loss scale, extra_inv)
PASS_ADAM = 4096 * 256 * 4                                                   # elements one pass of the grid-stride loop covers
PASS_MULTI = 64 * 1024
PASS_CHECK = 2048 * 256 * 4
PASS_REDUCE = 4096 * 256 * 8
GUARD = 16                                                                   # elements in front of and behind every buffer (64 / 32 bytes)
KERNELS = ["adam", "scaled", "multi"]


def _f(x):
    return float(np.float32(x))


TORCH_BETAS, TORCH_EPS = (_f(BETAS[0]), _f(BETAS[1])), _f(EPS)               # float32 torch gets the values the kernels get


def _api():
    from customnerf_amd._lib import lib, check, ptr, stream, AdamJobs, ADAM_MAX_JOBS
    return lib, check, ptr, stream, AdamJobs, ADAM_MAX_JOBS


class Guarded:
    """a device buffer of n elements, 16-byte aligned, with GUARD elements of a known pattern on both sides"""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.fill = 1234.5 if dtype == torch.float32 else 77.0
        self.whole = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + n]
        self.ptr = self.whole.data_ptr() + GUARD * self.whole.element_size()      # (an empty view has no data_ptr of its own)
        assert self.ptr % 16 == 0 and (n == 0 or self.t.data_ptr() == self.ptr)
        if init is None:
            self.t.zero_()
        else:
            self.set(init)

    def set(self, a):
        self.t.copy_(torch.as_tensor(np.ascontiguousarray(a)).to(self.t.dtype))

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == self.fill).all()) and bool((w[GUARD + self.t.numel():] == self.fill).all())


class Tensors:
    """p, g, m, v (+ the fp16 shadow) of one parameter tensor"""

    def __init__(self, n, with_half, p0=None, m0=None, v0=None):
        self.n = n
        self.p, self.g, self.m, self.v = Guarded(n, init=p0), Guarded(n), Guarded(n, init=m0), Guarded(n, init=v0)
        self.ph = Guarded(n, torch.float16) if with_half else None
        if with_half:
            self.ph.t.fill_(3.0)

    def all(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.ph) if b is not None]

    def half_ptr(self):
        return self.ph.ptr if self.ph is not None else None

    def assert_guards(self):
        for b in self.all():
            assert b.intact()

    def assert_half_is_p(self):
        if self.ph is not None:
            assert torch.equal(self.ph.t.view(torch.int16), self.p.t.half().view(torch.int16))


def _state(scale=65536.0, tracker=0.0, found=0.0, good=0.0):
    return torch.tensor([scale, tracker, found, good], dtype=torch.float32, device="cuda")


def _launch_adam(ts, lr, step, gs, zero_grad):
    lib, check, ptr, stream, _, _ = _api()
    check(lib.cnerf_adam_step(ts.p.ptr, ts.g.ptr, ts.m.ptr, ts.v.ptr, ts.half_ptr(), ts.n, lr, BETAS[0], BETAS[1], EPS, step, float(gs),
                              zero_grad, stream()), "adam_step")


def _launch_scaled(ts, lr, state, extra_inv, zero_grad):
    lib, check, ptr, stream, _, _ = _api()
    check(lib.cnerf_adam_step_scaled(ts.p.ptr, ts.g.ptr, ts.m.ptr, ts.v.ptr, ts.half_ptr(), ts.n, lr, BETAS[0], BETAS[1], EPS,
                                     ptr(state), extra_inv, zero_grad, stream()), "adam_step_scaled")


def _jobs(tensors, lrs):
    _, _, _, _, AdamJobs, _ = _api()
    jobs = AdamJobs()
    for j, (ts, lr) in enumerate(zip(tensors, lrs)):
        jobs.p[j], jobs.g[j], jobs.m[j], jobs.v[j] = ts.p.ptr, ts.g.ptr, ts.m.ptr, ts.v.ptr
        jobs.p_half[j] = ts.half_ptr()
        jobs.n[j], jobs.lr[j] = ts.n, lr
    jobs.n_jobs = len(tensors)
    return jobs


def _launch_multi(tensors, lrs, state, extra_inv, zero_grad, update_scaler, growth=2.0, backoff=0.5, interval=1 << 30):
    lib, check, ptr, stream, _, _ = _api()
    jobs = _jobs(tensors, lrs)
    check(lib.cnerf_adam_step_scaled_multi(ctypes.addressof(jobs), BETAS[0], BETAS[1], EPS, ptr(state), extra_inv, zero_grad, update_scaler,
                                           growth, backoff, interval, stream()), "adam_step_scaled_multi")


def _scaler_update(state, growth=2.0, backoff=0.5, interval=1 << 30):
    lib, check, ptr, stream, _, _ = _api()
    check(lib.cnerf_scaler_update(ptr(state), growth, backoff, interval, stream()), "scaler_update")


# ------------------------------------------------------------------------------------------------ the shared references (computed once)
_SEQ = {}


def _sequence(scale_key):
    """per size: the stored gradients of every step, the float64 reference (p, m, v, a) at every checkpoint, and float32 torch.optim.Adam's
    deviation from it on this device; then torch's worst deviation per checkpoint over all sizes.  Computed once per loss scale, never changed."""
    if scale_key in _SEQ:
        return _SEQ[scale_key]
    scale, extra_inv = SCALES[scale_key]
    gs = orr.gscale32(scale, extra_inv)
    seq = {"gs": gs, "sizes": {}, "torch": {c: [0.0, 0.0, 0.0] for c in CHECKPOINTS}}
    for i, (n, lr) in enumerate(zip(SIZES, LRS)):
        steps = max(CHECKPOINTS) if n == LONG_N else 5
        g = orr.stored_gradient(orr.gradient_mix(n, steps, seed=100 + i), scale)
        assert np.isfinite(g).all()
        gd = torch.from_numpy(g).cuda()
        tp = torch.zeros(n, device="cuda", requires_grad=True)
        opt = torch.optim.Adam([tp], lr=_f(lr), betas=TORCH_BETAS, eps=TORCH_EPS)
        p, m, v, a = (np.zeros(n) for _ in range(4))
        ref, tdev = {}, {}
        for s in range(1, steps + 1):
            p, m, v = orr.adam_reference(p, m, v, g[s - 1], lr, BETAS[0], BETAS[1], EPS, s, gs)
            a = orr.abs_moment_reference(a, g[s - 1], BETAS[0], gs)
            tp.grad = gd[s - 1] * float(gs)                                # GradScaler.unscale_: a float32 multiply by the float32 1/scale
            opt.step()
            if s in CHECKPOINTS:
                ref[s] = (p, m, v, a)
                st = opt.state[tp]
                tdev[s] = orr.adam_errors(tp.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), p, m, v, a, lr)
                seq["torch"][s] = [max(x, y) for x, y in zip(seq["torch"][s], tdev[s])]
        seq["sizes"][n] = dict(g=gd, ref=ref, torch=tdev, lr=lr, steps=steps)
    for c in CHECKPOINTS:
        assert all(x > 0 for x in seq["torch"][c])                           # float32 did round somewhere: there is a bound
    _SEQ[scale_key] = seq
    return seq


def _hold(tag, kernel_errs, torch_errs):
    """print both figures, then assert kernel <= BOUND * torch per quantity"""
    line = "  ".join(f"{q} {k:.2e}/{t:.2e}={k / t if t else float('inf'):.2f}" for q, k, t in zip(("dp/lr", "dv/v", "dm/a"), kernel_errs, torch_errs))
    print(f"{tag}: kernel/torch32 vs float64  {line}")
    for k, t in zip(kernel_errs, torch_errs):
        assert k <= BOUND * t, (tag, kernel_errs, torch_errs)


# ------------------------------------------------------------------------------------------------ 1. the three kernels against float64
@pytest.mark.parametrize("half_zero", [(True, 1), (False, 0)], ids=["half-zero_grad", "nohalf-keep_grad"])
@pytest.mark.parametrize("scale_key", list(SCALES))
@pytest.mark.parametrize("kernel", KERNELS)
def test_adam_kernels_against_float64(kernel, scale_key, half_zero):
    """Every size of SIZES over the gradient mix, 5 steps (300 for n = 4099, checked at 1, 5 and 300), the multi kernel as 8 + 3 jobs with one
    job of n = 0; errors against the float64 restatement within BOUND times float32 torch's; never-touched entries exactly zero; the fp16 shadow
    equal to p.half() bit for bit; g zeroed or left as it was; guards intact."""
    with_half, zero_grad = half_zero
    scale, extra_inv = SCALES[scale_key]
    seq = _sequence(scale_key)
    gs = seq["gs"]
    ts = {n: Tensors(n, with_half) for n in SIZES}
    empty = Tensors(0, with_half)
    state = _state(scale)
    worst = {c: [0.0, 0.0, 0.0] for c in CHECKPOINTS}
    first, second = SIZES[:7], SIZES[7:]                                      # 7 jobs + the empty one = the job limit; then the rest
    for s in range(1, max(CHECKPOINTS) + 1):
        live = [n for n in SIZES if s <= seq["sizes"][n]["steps"]]
        for n in live:
            ts[n].g.t.copy_(seq["sizes"][n]["g"][s - 1])
        if kernel == "adam":
            for n in live:
                _launch_adam(ts[n], seq["sizes"][n]["lr"], s, gs, zero_grad)
        elif kernel == "scaled":
            for n in live:
                _launch_scaled(ts[n], seq["sizes"][n]["lr"], state, extra_inv, zero_grad)
            _scaler_update(state)
        else:
            a = [n for n in first if n in live]
            if a:
                _launch_multi([ts[n] for n in a] + [empty], [seq["sizes"][n]["lr"] for n in a] + [1.0], state, extra_inv, zero_grad, 0)
            b = [n for n in second if n in live]
            _launch_multi([ts[n] for n in b], [seq["sizes"][n]["lr"] for n in b], state, extra_inv, zero_grad, 1)
        if s not in CHECKPOINTS:
            continue
        for n in live:
            t, info = ts[n], seq["sizes"][n]
            p, m, v = t.p.np(), t.m.np(), t.v.np()
            errs = orr.adam_errors(p, m, v, *info["ref"][s], info["lr"])
            worst[s] = [max(x, y) for x, y in zip(worst[s], errs)]
            _hold(f"{kernel} {scale_key} n={n} step {s}", errs, seq["torch"][s])
            never, _ = orr.mix_blocks(n)
            assert not p[:never].any() and not m[:never].any() and not v[:never].any()
            t.assert_half_is_p()
            if zero_grad:
                assert not t.g.np().any()
            else:
                assert torch.equal(t.g.t.view(torch.int32), info["g"][s - 1].view(torch.int32))
            t.assert_guards()
    if kernel != "adam":
        assert state.cpu().tolist() == [scale, float(max(CHECKPOINTS)), 0.0, float(max(CHECKPOINTS))]
    empty.assert_guards()
    for c in CHECKPOINTS:
        print(f"SUMMARY {kernel} {scale_key} step {c}: " + "  ".join(f"{k:.2e}/{t:.2e}" for k, t in zip(worst[c], seq["torch"][c])))


# ------------------------------------------------------------------------------------------------ one step from a state, shared by 2, 3 and 5
_ONE = {}


def _one_step_case(n, seed, k=0, lr=3e-3, scale_key="pow2", distinct_tail=0):
    """a state as `k` earlier steps would have left it (float32 p, m, v), this step's gradient, the float64 reference of step k + 1 and float32
    torch.optim.Adam's deviation from it on this device; computed once per case"""
    key = (n, seed, k, lr, scale_key, distinct_tail)
    if key in _ONE:
        return _ONE[key]
    scale, extra_inv = SCALES[scale_key]
    gs = orr.gscale32(scale, extra_inv)
    mix = orr.gradient_mix(n, 2, seed)
    if distinct_tail:                                                         # no other entry holds these values: a doubled or skipped update shows
        mix[1, n - distinct_tail:] = 50.0 + np.arange(distinct_tail) / 1024.0
        assert np.abs(mix[1, :n - distinct_tail]).max() < 50.0
    rng = np.random.default_rng(seed + 1)
    p0 = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    m0 = (0.1 * mix[0]).astype(np.float32)
    v0 = (0.01 * mix[0] ** 2).astype(np.float32)
    never, _ = orr.mix_blocks(n)
    p0[:never] = 0
    g = orr.stored_gradient(mix[1], scale)
    p, m, v = orr.adam_reference(p0, m0, v0, g, lr, BETAS[0], BETAS[1], EPS, k + 1, gs)
    a = orr.abs_moment_reference(np.abs(m0), g, BETAS[0], gs)
    tp = torch.from_numpy(p0).cuda().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=_f(lr), betas=TORCH_BETAS, eps=TORCH_EPS)
    opt.state[tp] = {"step": torch.tensor(float(k)), "exp_avg": torch.from_numpy(m0).cuda(), "exp_avg_sq": torch.from_numpy(v0).cuda()}
    tp.grad = torch.from_numpy(g).cuda() * float(gs)
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == k + 1
    tdev = orr.adam_errors(tp.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(), p, m, v, a, lr)
    case = dict(n=n, k=k, lr=lr, gs=gs, scale=scale, extra_inv=extra_inv, p0=p0, m0=m0, v0=v0, g=g, ref=(p, m, v, a), torch=tdev, never=never)
    _ONE[key] = case
    return case


def _tensors_of(case, with_half=True):
    ts = Tensors(case["n"], with_half, case["p0"], case["m0"], case["v0"])
    ts.g.set(case["g"])
    return ts


def _check_one_step(tag, case, ts, zero_grad=1):
    p, m, v = ts.p.np(), ts.m.np(), ts.v.np()
    _hold(tag, orr.adam_errors(p, m, v, *case["ref"], case["lr"]), case["torch"])
    nv = case["never"]
    assert not p[:nv].any() and not m[:nv].any() and not v[:nv].any()
    ts.assert_half_is_p()
    assert not ts.g.np().any() if zero_grad else np.array_equal(ts.g.np().view(np.uint32), case["g"].view(np.uint32))
    ts.assert_guards()


# ------------------------------------------------------------------------------------------------ 2. the second pass of each grid-stride loop
@pytest.mark.parametrize("kernel", KERNELS)
def test_adam_second_pass_of_the_grid_stride_loop(kernel):
    """n = one pass + 1029 (the vector body wraps, and the tail, one element here, starts behind it on the second pass); for the multi kernel
    n = one pass + 1 in one job, through the ABI.  The last 2000 gradients are like no others."""
    n = PASS_MULTI + 1 if kernel == "multi" else PASS_ADAM + 1029
    case = _one_step_case(n, seed=7, distinct_tail=2000)
    ts = _tensors_of(case)
    state = _state(case["scale"])
    if kernel == "adam":
        _launch_adam(ts, case["lr"], 1, case["gs"], 1)
    elif kernel == "scaled":
        _launch_scaled(ts, case["lr"], state, case["extra_inv"], 1)
    else:
        _launch_multi([ts], [case["lr"]], state, case["extra_inv"], 1, 1)
        assert state.cpu().tolist() == [case["scale"], 1.0, 0.0, 1.0]
    _check_one_step(f"{kernel} n={n}", case, ts)


# ------------------------------------------------------------------------------------------------ 3. the skipped step
def _snapshot(ts):
    return [b.whole.clone() for b in ts.all()]


def _assert_untouched(ts, snap, zero_grad):
    for b, before in zip(ts.all(), snap):
        bits = torch.int32 if b.whole.dtype == torch.float32 else torch.int16
        if b is ts.g and zero_grad:
            assert not b.t.any() and b.intact()
        else:
            assert torch.equal(b.whole.view(bits), before.view(bits))


@pytest.mark.parametrize("zero_grad", [1, 0])
@pytest.mark.parametrize("n", [PASS_ADAM + 1029, 3])
def test_skipped_step_of_the_scaled_kernel_touches_nothing(n, zero_grad):
    """found_inf = 1: p, m, v and the fp16 shadow keep their bits, element by element; g is cleared (zero_grad = 1) or kept; the state is only read"""
    case = _one_step_case(n, seed=8)
    ts = _tensors_of(case)
    ts.g.t[n // 2] = float("inf")
    snap = _snapshot(ts)
    state = _state(case["scale"], 3.0, 1.0, 41.0)
    _launch_scaled(ts, case["lr"], state, case["extra_inv"], zero_grad)
    _assert_untouched(ts, snap, zero_grad)
    assert state.cpu().tolist() == [case["scale"], 3.0, 1.0, 41.0]


@pytest.mark.parametrize("update_scaler", [1, 0])
@pytest.mark.parametrize("zero_grad", [1, 0])
def test_skipped_step_of_the_multi_kernel_touches_nothing(zero_grad, update_scaler):
    """three jobs, one spanning several workgroups; with update_scaler the scale backs off once, flag and tracker clear, good_steps stays"""
    cases = [_one_step_case(n, seed=9 + n) for n in (5000, 3, 1025)]
    tss = [_tensors_of(c) for c in cases]
    tss[0].g.t[4999] = float("nan")
    snaps = [_snapshot(t) for t in tss]
    state = _state(1024.0, 3.0, 1.0, 41.0)
    _launch_multi(tss, [c["lr"] for c in cases], state, 1.0, zero_grad, update_scaler, 2.0, 0.5, 4)
    for t, s in zip(tss, snaps):
        _assert_untouched(t, s, zero_grad)
    assert state.cpu().tolist() == ([512.0, 0.0, 0.0, 41.0] if update_scaler else [1024.0, 3.0, 1.0, 41.0])


# ------------------------------------------------------------------------------------------------ 4. the ticket of the multi-tensor launch
def test_multi_launch_ticket_applies_one_update_per_launch():
    """three launches back to back on one stream, five workgroups each: whichever workgroup finishes last applies GradScaler.update() once, and
    the ticket is back at zero for the next launch; so is it after a launch without jobs"""
    n = 5000
    assert -(-n // 1024) == 5
    case = _one_step_case(n, seed=21)
    ts = _tensors_of(case, with_half=False)
    state = _state(1024.0, 0.0, 0.0, 0.0)
    hist = torch.zeros(5, 4, device="cuda")
    for i in range(3):
        _launch_multi([ts], [case["lr"]], state, 1.0, 0, 1, 2.0, 0.5, 2)
        hist[i].copy_(state)                                                   # on the same stream: nothing waits for the host in between
    _launch_multi([], [], state, 1.0, 0, 1, 2.0, 0.5, 2)
    hist[3].copy_(state)
    state[2] = 1.0
    _launch_multi([], [], state, 1.0, 0, 1, 2.0, 0.5, 2)
    hist[4].copy_(state)
    want, st = [], np.array([1024.0, 0, 0, 0], dtype=np.float32)
    for i in range(5):
        st[2] = 1.0 if i == 4 else 0.0
        st = orr.scaler_reference(st, 2.0, 0.5, 2)
        want.append(st.copy())
    assert hist.cpu().numpy().tobytes() == np.stack(want).tobytes(), (hist.cpu().numpy(), want)
    assert [w[3] for w in want] == [1, 2, 3, 4, 4] and [w[0] for w in want] == [1024, 2048, 2048, 4096, 2048]
    ts.assert_guards()


# ------------------------------------------------------------------------------------------------ 5. bias correction late in training
@pytest.mark.parametrize("k", [0, 9, 999, 99999, 16777214])
@pytest.mark.parametrize("kernel", ["scaled", "multi"])
def test_bias_correction_after_k_good_steps(kernel, k):
    """DynamicLossScaler.set_good_steps(k), then one step: the kernels take step = k + 1 from the state, against float64 with that step;
    good_steps is k + 1 afterwards.  (The counter is a float32: it stops counting at 2^24 = 16 777 216, so nothing is asserted beyond
    16 777 215; training runs are four orders of magnitude shorter.)"""
    from customnerf_amd.optim import DynamicLossScaler
    case = _one_step_case(1025, seed=30, k=k)
    ts = _tensors_of(case)
    sc = DynamicLossScaler("cuda", init_scale=case["scale"], growth_interval=1 << 30)
    sc.set_good_steps(k)
    if kernel == "scaled":
        _launch_scaled(ts, case["lr"], sc.state, case["extra_inv"], 1)
        sc.update()
    else:
        _launch_multi([ts], [case["lr"]], sc.state, case["extra_inv"], 1, 1)
    _check_one_step(f"{kernel} k={k}", case, ts)
    assert sc.good_steps() == k + 1 and sc.state.cpu().tolist() == [case["scale"], 1.0, 0.0, float(k + 1)]


# ------------------------------------------------------------------------------------------------ 6. the scaler update
@pytest.mark.parametrize("via", ["scaler_update", "multi_tail"])
@pytest.mark.parametrize("script", orr.SCALER_SCRIPTS, ids=[s[0] for s in orr.SCALER_SCRIPTS])
def test_scaler_update_follows_the_scripts(script, via):
    """the scripted sequences of the host test (where torch._amp_update_scale_ walks them): the state after every step equals
    scaler_reference's exactly.  Non-finite steps raise the flag through cnerf_scaler_check on a gradient buffer that holds the value."""
    lib, check, ptr, stream, _, _ = _api()
    _, init, growth, backoff, interval, events = script
    want = orr.run_scaler_script(script)
    state = torch.tensor(init, dtype=torch.float32, device="cuda")
    hist = torch.zeros(len(events), 4, device="cuda")
    grads = {e: torch.tensor([1.0, val, -2.0, 0.5, 3.0], device="cuda") for e, val in orr.EVENT_VALUE.items()}
    grads["c"] = torch.tensor([1.0, 3e38, -2.0, 0.5, 3.0], device="cuda")
    for i, e in enumerate(events):
        check(lib.cnerf_scaler_check(ptr(grads[e]), 5, ptr(state), stream()), "scaler_check")
        if via == "scaler_update":
            check(lib.cnerf_scaler_update(ptr(state), growth, backoff, interval, stream()), "scaler_update")
        else:
            _launch_multi([], [], state, 1.0, 1, 1, growth, backoff, interval)
        hist[i].copy_(state)
    got = hist.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (script[0], via, got, want)


def test_scaler_growth_stops_at_the_largest_finite_scale():
    """scale 2^127, tracker one below the interval, a clean step: torch keeps the scale (2^128 is not a float32), resets the tracker and counts
    the step.  Before the guard in cn_scaler_update the scale became inf here, and no later backoff (inf * 0.5) brought it back."""
    for via in ("scaler_update", "multi_tail"):
        state = _state(2.0 ** 127, 1999.0, 0.0, 7.0)
        if via == "scaler_update":
            _scaler_update(state, 2.0, 0.5, 2000)
        else:
            _launch_multi([], [], state, 1.0, 1, 1, 2.0, 0.5, 2000)
        got = state.cpu().tolist()
        print(f"{via}: state after growth at 2^127: {got}")
        assert got == [2.0 ** 127, 0.0, 0.0, 8.0], (via, got)
        assert got == list(orr.scaler_reference([2.0 ** 127, 1999.0, 0.0, 7.0], 2.0, 0.5, 2000))


# ------------------------------------------------------------------------------------------------ 7. the non-finite check
def test_scaler_check_finds_one_bad_value_anywhere():
    lib, check, ptr, stream, _, _ = _api()
    n = PASS_CHECK + 1027
    rng = np.random.default_rng(40)
    host = np.where(rng.random(n) < 0.5, 3e38, -3e38).astype(np.float32)
    sub = rng.random(n) < 0.25
    host[sub] = (rng.integers(1, 1 << 23, size=int(sub.sum())).astype(np.uint32) | (rng.integers(0, 2, size=int(sub.sum())).astype(np.uint32) << 31)).view(np.float32)
    assert np.isfinite(host).all() and (np.abs(host[sub]) < 1.2e-38).all()
    buf = Guarded(n, init=host)
    buf.whole[:GUARD] = float("inf")                                           # what lies outside the buffer is not looked at
    buf.whole[GUARD + n:] = float("nan")
    state = _state(65536.0, 5.0, 0.0, 9.0)

    def run(t=buf.t, count=n):
        check(lib.cnerf_scaler_check(ptr(t), count, ptr(state), stream()), "scaler_check")
        return state.cpu().tolist()

    assert run() == [65536.0, 5.0, 0.0, 9.0]                                   # +-3e38 and subnormals: all finite
    # index 0; the last element of the last vector of the first pass; the first element of the second pass; the last tail element
    for pos in (0, PASS_CHECK - 1, PASS_CHECK, n - 1):
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = float(buf.t[pos])
            buf.t[pos] = bad
            assert run() == [65536.0, 5.0, 1.0, 9.0], (pos, bad)
            buf.t[pos] = keep
            assert run() == [65536.0, 5.0, 1.0, 9.0]                           # a clean check does not clear a raised flag
            state[2] = 0.0
            assert run() == [65536.0, 5.0, 0.0, 9.0], (pos, bad)               # ... and the buffer is clean again
    for small in (1, 3):
        for bad in (float("inf"), float("-inf"), float("nan")):
            t = Guarded(small, init=np.full(small, -3e38, dtype=np.float32))
            t.whole[:GUARD] = float("nan")
            t.whole[GUARD + small:] = float("inf")
            assert run(t.t, small)[2] == 0.0
            t.t[small - 1] = bad
            assert run(t.t, small)[2] == 1.0
            state[2] = 0.0


# ------------------------------------------------------------------------------------------------ 8. pack
def _pack(src_host, scale):
    lib, check, ptr, stream, _, _ = _api()
    n = src_host.size
    g, out = Guarded(n, init=src_host), Guarded(n, torch.float16)
    out.t.fill_(5.0)
    want_torch = (g.t * scale).half().cpu().numpy()
    check(lib.cnerf_dp_pack(ptr(g.t), ptr(out.t), n, scale, stream()), "dp_pack")
    got = out.np()
    assert not g.np().any() and g.intact() and out.intact()                    # the source is zeroed (+0), nothing else is touched
    assert not np.signbit(g.np()).any()
    return got, want_torch


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_dp_pack_random_values_over_two_passes(scale):
    n = PASS_ADAM + 1029
    rng = np.random.default_rng(50)
    src = (rng.standard_normal(n) * 10.0 ** rng.integers(-9, 8, size=n)).astype(np.float32)
    got, want_torch = _pack(src, scale)
    want = orr.pack_reference(src, scale)
    assert np.isinf(want).any() and (want == 0).any() and ((np.abs(want) < 6e-5) & (want != 0)).any()      # overflow, underflow and subnormals occur
    assert orr.same_halves(got, want) and orr.same_halves(got, want_torch)


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_dp_pack_float16_edges_in_body_and_tail(scale):
    """n = 67: 16 vectors and a tail of 3.  Every edge value stands in the vector body, and, three at a time, in the tail."""
    vals, bits = orr.half_edges()
    src_edges = (vals / np.float32(scale)).astype(np.float32)                 # a power of two: the product is the edge value again
    assert vals.size <= 64
    for r in range(0, vals.size, 3):
        src = np.full(67, 1.0, dtype=np.float32)
        src[:vals.size] = src_edges
        tail = src_edges[r:r + 3]
        src[64:64 + tail.size] = tail
        got, want_torch = _pack(src, scale)
        assert orr.same_halves(got, orr.pack_reference(src, scale)) and orr.same_halves(got, want_torch), (r, got.view(np.uint16))
        for v, h, b in list(zip(vals, got.view(np.uint16), bits)) + list(zip(vals[r:r + 3], got.view(np.uint16)[64:], bits[r:r + 3])):
            is_nan = (h & 0x7C00) == 0x7C00 and (h & 0x3FF) != 0
            assert is_nan if b is None else h == b, (float(v), hex(h), b)


def test_dp_pack_rounds_the_product_to_float32_first():
    """scale 1/3: products whose float32 rounding lands on a tie between two halves, so that rounding the exact product to float16 at once
    (what a fused multiply-convert does) gives the neighbouring half.  In the vector body and in the tail, which must round alike."""
    scale = float(np.float32(1.0 / 3.0))
    rng = np.random.default_rng(51)
    x = (rng.standard_normal(1 << 22) * 10.0 ** rng.integers(-3, 4, size=1 << 22)).astype(np.float32)
    twice = orr.pack_reference(x, scale)
    once = (x.astype(np.float64) * scale).astype(np.float16)                  # the float64 product of two float32 is exact
    pick = x[twice.view(np.uint16) != once.view(np.uint16)]
    assert pick.size >= 6, pick.size
    src = np.full(67, 1.0, dtype=np.float32)
    src[:3], src[64:] = pick[:3], pick[3:6]
    got, want_torch = _pack(src, scale)
    assert orr.same_halves(got, orr.pack_reference(src, scale)) and orr.same_halves(got, want_torch), (src, got.view(np.uint16))


# ------------------------------------------------------------------------------------------------ 9. reduce
def _reduce(recv_host, world, with_state=True):
    lib, check, ptr, stream, _, _ = _api()
    shard = recv_host.shape[1]
    recv = torch.from_numpy(recv_host.view(np.int16)).cuda().view(torch.float16)
    out = Guarded(shard)
    out.t.fill_(-1.0)
    state = _state(65536.0, 5.0, 0.0, 9.0)
    check(lib.cnerf_dp_reduce(ptr(recv), world, shard, ptr(out.t), ptr(state) if with_state else None, stream()), "dp_reduce")
    assert out.intact() and torch.equal(recv.cpu().view(torch.int16), torch.from_numpy(recv_host.view(np.int16)))
    return out.np(), state.cpu().tolist()


def _assert_reduced(recv, world, flag):
    got, state = _reduce(recv, world)
    want, want_flag = orr.reduce_reference(recv, world)
    assert want_flag == flag and got.tobytes() == want.tobytes()              # exact, NaN bits and signed zeros included
    assert state == [65536.0, 5.0, 1.0 if flag else 0.0, 9.0]


def test_dp_reduce_two_passes():
    shard, world = PASS_REDUCE + 64, 2
    rng = np.random.default_rng(60)
    recv = (rng.standard_normal((world, shard), dtype=np.float32) * (10.0 ** rng.integers(-6, 4, size=(world, shard))).astype(np.float32)).astype(np.float16)
    recv[:, -64:] = (np.arange(128).reshape(2, 64) + 1000).astype(np.float16)                            # the second pass's elements are like no others
    _assert_reduced(recv, world, False)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_dp_reduce_small_shards_and_the_flag(world):
    rng = np.random.default_rng(61 + world)
    base = (rng.standard_normal((world, 64)) * 10.0 ** rng.integers(-7, 4, size=(world, 64))).astype(np.float16)
    base[0, 5], base[world - 1, 6] = -0.0, -0.0
    _assert_reduced(base, world, False)
    full = np.full((world, 64), 65504.0, dtype=np.float16)                   # the largest halves from every rank: the float32 sum is finite
    _assert_reduced(full, world, False)
    for r, i in ((0, 0), (world - 1, 63), (world // 2, 31)):
        bad = base.copy()
        bad[r, i] = np.inf
        _assert_reduced(bad, world, True)
    if world > 1:
        bad = base.copy()
        bad[0, 17], bad[world - 1, 17] = np.inf, -np.inf                     # inf + (-inf) = NaN
        _assert_reduced(bad, world, True)
        got, _ = _reduce(bad, world)
        assert np.isnan(got[17])
    # a null state pointer: the sum is written, nothing else (the kernel tests the pointer)
    got, state = _reduce(base, world, with_state=False)
    assert got.tobytes() == orr.reduce_reference(base, world)[0].tobytes() and state == [65536.0, 5.0, 0.0, 9.0]


# ------------------------------------------------------------------------------------------------ 10. argument checks
def test_argument_checks():
    lib, check, ptr, stream, AdamJobs, max_jobs = _api()
    from customnerf_amd.optim import adam_step
    assert max_jobs == 8
    n = 64
    bufs = {k: torch.full((n + 8,), 2.0, device="cuda") for k in "pgmv"}
    half = torch.full((n + 8,), 2.0, dtype=torch.float16, device="cuda")
    state = _state()

    def args(off=None, half_off=0, count=n):
        t = {k: (b[1:1 + count] if k == off else b[:count]) for k, b in bufs.items()}
        return t["p"], t["g"], t["m"], t["v"], half[half_off:half_off + count]

    def untouched():
        return all(bool((b == 2.0).all()) for b in bufs.values()) and bool((half == 2.0).all())

    for off in "pgmv":                                                        # 4 bytes off 16-byte alignment
        p, g, m, v, ph = args(off)
        with pytest.raises(ValueError):
            adam_step(p, g, m, v, 1e-3, step=1, p_half=ph)
        assert lib.cnerf_adam_step_scaled(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ph), n, 1e-3, 0.9, 0.99, 1e-15, ptr(state), 1.0, 1, stream()) < 0
    p, g, m, v, ph = args(half_off=1)                                         # the shadow 2 bytes off 8-byte alignment
    with pytest.raises(ValueError):
        adam_step(p, g, m, v, 1e-3, step=1, p_half=ph)
    assert lib.cnerf_adam_step_scaled(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ph), n, 1e-3, 0.9, 0.99, 1e-15, ptr(state), 1.0, 1, stream()) < 0
    p, g, m, v, ph = args()
    with pytest.raises(ValueError):
        adam_step(p, g, m, v, 1e-3, step=0, p_half=ph)
    # n = 0 is a success that writes nothing, even through misaligned pointers
    assert lib.cnerf_adam_step(ptr(p) + 4, ptr(g), ptr(m), ptr(v), ptr(ph) + 2, 0, 1e-3, 0.9, 0.99, 1e-15, 1, 1.0, 1, stream()) == 0
    assert lib.cnerf_adam_step_scaled(ptr(p) + 4, ptr(g), ptr(m), ptr(v), ptr(ph) + 2, 0, 1e-3, 0.9, 0.99, 1e-15, ptr(state), 1.0, 1, stream()) == 0
    assert lib.cnerf_scaler_check(ptr(g), 0, ptr(state), stream()) == 0
    assert lib.cnerf_dp_pack(ptr(g), ptr(half), 0, 1.0, stream()) == 0
    assert lib.cnerf_dp_reduce(ptr(half), 2, 0, ptr(p), ptr(state), stream()) == 0
    jobs = AdamJobs()
    jobs.n_jobs = 9
    assert lib.cnerf_adam_step_scaled_multi(ctypes.addressof(jobs), 0.9, 0.99, 1e-15, ptr(state), 1.0, 1, 1, 2.0, 0.5, 2000, stream()) < 0
    jobs.n_jobs = 0
    for growth, backoff, interval in ((0.5, 0.5, 2000), (2.0, 0.0, 2000), (2.0, 1.5, 2000), (2.0, -0.5, 2000), (2.0, 0.5, 0), (float("nan"), 0.5, 2000)):
        assert lib.cnerf_scaler_update(ptr(state), growth, backoff, interval, stream()) < 0
        assert lib.cnerf_adam_step_scaled_multi(ctypes.addressof(jobs), 0.9, 0.99, 1e-15, ptr(state), 1.0, 1, 1, growth, backoff, interval, stream()) < 0
    assert lib.cnerf_dp_reduce(ptr(half), 0, 64, ptr(p), ptr(state), stream()) < 0
    assert lib.cnerf_scaler_check(ptr(bufs["g"][1:]), n, ptr(state), stream()) < 0
    assert lib.cnerf_dp_pack(ptr(bufs["g"][1:]), ptr(half), n, 1.0, stream()) < 0
    torch.cuda.synchronize()
    assert untouched() and state.cpu().tolist() == [65536.0, 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ FusedAdam: parameters that are not contiguous
def _fused(p, scaler):
    from customnerf_amd.optim import FusedAdam
    opt = FusedAdam([p], lr=1e-2)
    opt.scaler = scaler
    return opt


@pytest.mark.parametrize("with_scaler", [False, True])
def test_fused_adam_rejects_a_gradient_laid_out_unlike_its_parameter(with_scaler):
    """a contiguous .grad on a transposed parameter: the kernel would pair element k of one with element k of the other in memory order"""
    from customnerf_amd.optim import DynamicLossScaler
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(6, 8, device="cuda").t())
    assert not p.is_contiguous()
    p.grad = torch.randn(8, 6, device="cuda")
    before = p.detach().clone()
    opt = _fused(p, DynamicLossScaler("cuda", init_scale=1.0) if with_scaler else None)
    with pytest.raises(ValueError, match="wrong order"):
        opt.step()
    assert torch.equal(p.detach(), before)


@pytest.mark.parametrize("with_scaler", [False, True])
def test_fused_adam_steps_a_dense_transposed_parameter(with_scaler):
    """parameter and gradient both transposed the same way (what autograd produces): every element meets its own gradient"""
    from customnerf_amd.optim import DynamicLossScaler
    rng = np.random.default_rng(70)
    p0 = (rng.standard_normal((8, 6)) * 1e-2).astype(np.float32)
    g = rng.standard_normal((3, 8, 6)).astype(np.float32)

    def transposed(a):                                                        # logical [8, 6], stored as [6, 8]
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()

    p = torch.nn.Parameter(transposed(p0))
    opt = _fused(p, DynamicLossScaler("cuda", init_scale=1.0) if with_scaler else None)
    rp, rm, rv = p0.astype(np.float64), np.zeros((8, 6)), np.zeros((8, 6))
    for s in range(3):
        p.grad = transposed(g[s])
        assert p.grad.stride() == p.stride() and not p.is_contiguous()
        opt.step()
        if with_scaler:
            opt.scaler.update()
        rp, rm, rv = orr.adam_reference(rp, rm, rv, g[s], 1e-2, 0.9, 0.99, 1e-15, s + 1, 1.0)
    # |p| < 0.1 and three steps of at most lr each: a float32 p is within a few ulp(0.1) = 7.5e-9 of the float64 one; paired with the wrong
    # gradient an element moves the other way in one step out of two: 1e-2 and more
    assert np.abs(p.detach().cpu().numpy() - rp).max() < 1e-7
    st = opt.state[p]
    assert np.abs(st["exp_avg"].cpu().numpy() - rm).max() < 1e-6 and np.abs(st["exp_avg_sq"].cpu().numpy() - rv).max() < 1e-6
