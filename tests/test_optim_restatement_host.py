"""CPU: the float64 restatement of the optimiser path (tests/optim_restatement.py) against torch's own implementations, so that what
tests/test_gpu_optim.py holds the HIP kernels to is itself pinned: adam_reference against torch.optim.Adam on float64 tensors,
scaler_reference against torch._amp_update_scale_, pack_reference against numpy's float16 cast, reduce_reference against a float64 sum."""
import numpy as np
import torch

import optim_restatement as orr

BETAS, EPS = (0.9, 0.99), 1e-15


def _f(x):
    return float(np.float32(x))


def test_adam_reference_matches_torch_adam_in_float64():
    """300 steps of the gradient mix; p, m and v to 1e-12.  m and p are sums that cancel (the alternating block most of all), so their error is
    taken against the size of what was summed: the |g'|-driven moment for m, the travelled distance sum |dp| for p; v is plain relative."""
    n, steps, lr, scale, extra_inv = 4099, 300, 1e-2, 3000.0, 1.0 / 3.0
    gs = orr.gscale32(scale, extra_inv)
    gp = orr.gradient_mix(n, steps, seed=11)
    p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=_f(lr), betas=(_f(BETAS[0]), _f(BETAS[1])), eps=_f(EPS))
    rp, rm, rv, ra, travelled = (np.zeros(n) for _ in range(5))
    never, alt = orr.mix_blocks(n)
    for s in range(steps):
        g = orr.stored_gradient(gp[s], scale)
        p.grad = torch.from_numpy(g.astype(np.float64) * float(gs))
        opt.step()
        before = rp
        rp, rm, rv = orr.adam_reference(rp, rm, rv, g, lr, BETAS[0], BETAS[1], EPS, s + 1, gs)
        ra = orr.abs_moment_reference(ra, g, BETAS[0], gs)
        travelled += np.abs(rp - before)
    st = opt.state[p]
    tp, tm, tv = p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
    assert (rv[never:] > 0).all() and (ra[never:] > 0).all() and (travelled[never:] > 0).all()
    live = slice(never, None)
    ep = float(np.max(np.abs(tp - rp)[live] / travelled[live]))
    em = float(np.max(np.abs(tm - rm)[live] / ra[live]))
    ev = float(np.max(np.abs(tv - rv)[live] / rv[live]))
    print(f"float64 torch.optim.Adam vs adam_reference after {steps} steps: p {ep:.2e}  m {em:.2e}  v {ev:.2e}")
    assert ep <= 1e-12 and em <= 1e-12 and ev <= 1e-12, (ep, em, ev)
    # the alternating block did cancel, and the never-touched block never moved, in both
    ratio = np.abs(rm[never:]) / ra[never:]
    assert float(np.median(ratio[:alt])) < float(np.median(ratio[alt:]))
    for a in (rp, rm, rv, tp, tm, tv):
        assert not a[:never].any()


def test_adam_reference_takes_its_inputs_at_float32():
    p, m, v = orr.adam_reference([0.0], [0.0], [0.0], np.array([0.25], dtype=np.float32), 0.1, 0.9, 0.99, 1e-15, 1, 1.0)
    b1, b2, lr = float(np.float32(0.9)), float(np.float32(0.99)), float(np.float32(0.1))
    assert m[0] == (1 - b1) * 0.25 and v[0] == (1 - b2) * 0.25 * 0.25 and m.dtype == np.float64
    assert abs(p[0] + lr) < 1e-13 * lr and p[0] != -0.1                    # the first step moves by lr (eps aside), the float32 lr


def _torch_scaler_script(script):
    _, state, growth, backoff, interval, events = script
    scale, tracker = torch.tensor([state[0]], dtype=torch.float32), torch.tensor([int(state[1])], dtype=torch.int32)
    good, out = int(state[3]), []
    for e in events:
        found = torch.zeros(1)
        if e != "c":
            # GradScaler.unscale_: the non-finite check of the step's gradients raises found_inf
            grads = [torch.tensor([1.0, orr.EVENT_VALUE[e], -2.0])]
            torch._amp_foreach_non_finite_check_and_unscale_(grads, found, torch.ones(1))
        assert float(found) == (0.0 if e == "c" else 1.0)
        torch._amp_update_scale_(scale, tracker, found, float(growth), float(backoff), int(interval))
        good += int(e == "c")                                              # GradScaler.step() skips optimizer.step() when found_inf
        out.append([float(scale), float(tracker), 0.0, float(good)])
    return np.array(out, dtype=np.float32)


def test_scaler_reference_matches_torch_amp_update_scale():
    for script in orr.SCALER_SCRIPTS:
        ours, theirs = orr.run_scaler_script(script), _torch_scaler_script(script)
        assert ours.tobytes() == theirs.tobytes(), (script[0], ours, theirs)
    mixed = orr.run_scaler_script(orr.SCALER_SCRIPTS[0])
    assert list(mixed[:9, 0]) == [1024] * 3 + [2048] * 4 + [4096] * 2      # two growth boundaries
    assert mixed[9, 0] == 2048 and mixed[10, 0] == 1024 and mixed[12, 0] == 512 and mixed[16, 0] == 1024 and mixed[17, 0] == 512      # backoff directly after a growth
    top = orr.run_scaler_script(orr.SCALER_SCRIPTS[3])
    assert list(top[0]) == [2.0 ** 127, 0, 0, 8] and np.isfinite(top[:, 0]).all() and top[5, 0] == 2.0 ** 126 and top[9, 0] == 2.0 ** 127


def test_scaler_reference_counts_applied_steps_only_and_stops_at_2_24():
    st = orr.scaler_reference([8.0, 0, 1, 41], 2.0, 0.5, 100)
    assert list(st) == [4.0, 0, 0, 41]
    st = orr.scaler_reference([8.0, 5, 0, 41], 2.0, 0.5, 100)
    assert list(st) == [8.0, 6, 0, 42]
    assert orr.scaler_reference([8.0, 0, 0, 2.0 ** 24 - 2], 2.0, 0.5, 100)[3] == 2.0 ** 24 - 1
    assert orr.scaler_reference([8.0, 0, 0, 2.0 ** 24], 2.0, 0.5, 100)[3] == 2.0 ** 24          # a float32 counter: 2^24 + 1 is not a float32


def test_pack_reference_matches_numpy_float16():
    vals, bits = orr.half_edges()
    for scale in (1.0, 0.125):
        src = (vals / np.float32(scale)).astype(np.float32)               # a power of two: the product is the edge value again
        got = orr.pack_reference(src, scale)
        with np.errstate(over="ignore"):
            want = (src * np.float32(scale)).astype(np.float16)
        assert orr.same_halves(got, want), (scale, got.view(np.uint16), want.view(np.uint16))
        for v, h, b in zip(vals, got.view(np.uint16), bits):
            is_nan = (h & 0x7C00) == 0x7C00 and (h & 0x3FF) != 0
            assert is_nan if b is None else h == b, (v, hex(h), b)           # and the bit patterns worked out by hand
    # every float16 bit pattern comes back from its own float32 value, and random float32 of every magnitude rounds as numpy rounds
    allh = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    assert orr.same_halves(orr.pack_reference(allh.astype(np.float32), 1.0), allh)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(1 << 18) * 10.0 ** rng.integers(-9, 6, size=1 << 18)).astype(np.float32)
    for scale in (1.0, 0.125, 1.0 / 3.0):
        with np.errstate(over="ignore"):
            want = (x * np.float32(scale)).astype(np.float16)
        assert orr.same_halves(orr.pack_reference(x, scale), want)
    # midpoints between neighbouring halves (ties) and their float32 neighbours on both sides
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(np.float32)
    for t in (mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9)), -mid):
        assert orr.same_halves(orr.pack_reference(t, 1.0), t.astype(np.float16))


def test_reduce_reference_is_the_exact_rank_ordered_sum():
    rng = np.random.default_rng(6)
    for world in (1, 3, 8):
        recv = (rng.standard_normal((world, 64)) * 10.0 ** rng.integers(-6, 4, size=(world, 64))).astype(np.float16)
        out, flag = orr.reduce_reference(recv, world)
        acc = np.zeros(64, dtype=np.float32)
        for r in range(world):
            acc = (acc.astype(np.float64) + recv[r].astype(np.float64)).astype(np.float32)      # a float32 add is the rounded exact sum
        assert out.dtype == np.float32 and out.tobytes() == acc.tobytes() and flag is False
    full = np.full((8, 64), 65504.0, dtype=np.float16)
    out, flag = orr.reduce_reference(full, 8)
    assert flag is False and (out == 8 * 65504.0).all()
    full[3, 7] = np.inf
    assert orr.reduce_reference(full, 8)[1] is True
    full[5, 7] = -np.inf
    out, flag = orr.reduce_reference(full, 8)
    assert flag is True and np.isnan(out[7])
