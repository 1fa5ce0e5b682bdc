"""The optimiser path restated in plain numpy, float64 where the rule is arithmetic and bit manipulation where it is a number format: what
k_adam / k_adam_scaled / k_adam_scaled_multi, k_scaler_update, k_dp_pack and k_dp_reduce (customnerf_amd/csrc/misc.hip, optim_common.h) are
held to by tests/test_gpu_optim.py, and what tests/test_optim_restatement_host.py holds to torch on the CPU.  No torch, no project imports.

Also the inputs both test modules share: the gradient mix, the float16 edge list and the scaler scripts."""
import numpy as np

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ Adam
def f32_inputs(lr, beta1, beta2, eps, gscale):
    """the rule's float32 inputs at their float32 values, as doubles"""
    return tuple(F64(F32(x)) for x in (lr, beta1, beta2, eps, gscale))


def adam_reference(p, m, v, g, lr, beta1, beta2, eps, step, gscale=1.0):
    """torch.optim.Adam's rule (no weight decay, no amsgrad), float64 throughout -> (p, m, v), new arrays.
    `g` is the stored float32 gradient, g' = g * gscale the one the rule sees; lr, the betas, eps and gscale are taken at their float32 values
    (they cross the ABI as floats; the scaled kernels' gscale is the float32 quotient extra_inv / scale), everything after that is double."""
    lr, beta1, beta2, eps, gscale = f32_inputs(lr, beta1, beta2, eps, gscale)
    p, m, v = (np.array(x, dtype=F64) for x in (p, m, v))
    gk = np.asarray(np.asarray(g, dtype=F32), dtype=F64) * gscale
    bc1 = 1.0 - beta1 ** F64(step)
    bc2 = 1.0 - beta2 ** F64(step)
    m = beta1 * m + (1.0 - beta1) * gk
    v = beta2 * v + (1.0 - beta2) * gk * gk
    p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return p, m, v


def abs_moment_reference(a, g, beta1, gscale=1.0):
    """the first-moment recurrence driven by |g'|: the scale an error of m is measured against (m itself cancels where the sign alternates)"""
    beta1, gscale = F64(F32(beta1)), F64(F32(gscale))
    return beta1 * np.asarray(a, dtype=F64) + (1.0 - beta1) * np.abs(np.asarray(np.asarray(g, dtype=F32), dtype=F64) * gscale)


def adam_errors(p, m, v, p_ref, m_ref, v_ref, a_ref, lr):
    """-> (max |dp| / lr, max |dv| / v_ref over v_ref > 0, max |dm| / a_ref over a_ref > 0), against the float64 reference"""
    lr = F64(F32(lr))
    p, m, v = (np.asarray(x, dtype=F64) for x in (p, m, v))
    ep = float(np.max(np.abs(p - p_ref)) / lr) if p.size else 0.0
    vm, am = v_ref > 0, a_ref > 0
    ev = float(np.max(np.abs(v - v_ref)[vm] / v_ref[vm])) if vm.any() else 0.0
    em = float(np.max(np.abs(m - m_ref)[am] / a_ref[am])) if am.any() else 0.0
    return ep, ev, em


# ---- the gradient mix: randn * 10^k (k in -6..0, one k per entry), 30 % exact zeros redrawn every step, a leading block that never receives a
# gradient, then a block whose sign alternates every step (never zeroed, so m cancels as hard as it can); |g'| >= 1e-12 wherever it is not zero
MIX_LEAD = 64


def mix_blocks(n):
    """-> (never, alt): the number of leading entries without any gradient and of alternating-sign entries after them"""
    return min(MIX_LEAD, n // 4), min(MIX_LEAD, n // 4)


def gradient_mix(n, steps, seed):
    """-> float64 [steps, n] of g' (the unscaled gradients)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(-6, 1, size=n)
    never, alt = mix_blocks(n)
    out = np.empty((steps, n), dtype=F64)
    for s in range(steps):
        g = rng.standard_normal(n) * 10.0 ** k
        g = np.where(np.abs(g) < 1e-12, np.copysign(1e-12, g), g)
        g[rng.random(n) < 0.3] = 0.0
        a = slice(never, never + alt)
        mag = np.abs(rng.standard_normal(alt)) * 10.0 ** k[a]
        g[a] = np.maximum(mag, 1e-12) * (1.0 if s % 2 == 0 else -1.0)
        g[:never] = 0.0
        out[s] = g
    return out


def stored_gradient(gp, scale):
    """what the backward of the scaled loss leaves in the float32 gradient buffer"""
    return np.asarray(np.asarray(gp, dtype=F64) * F64(scale), dtype=F32)


def gscale32(scale, extra_inv):
    """cn_scaler_gscale: the float32 quotient"""
    return F32(F32(extra_inv) / F32(scale))


# ------------------------------------------------------------------------------------------------ loss scaler
def scaler_reference(state, growth, backoff, interval):
    """torch.cuda.amp.GradScaler.update() on float32 {scale, growth_tracker, found_inf, good_steps} -> the new float32[4].
    found_inf: the scale backs off and the tracker restarts; else the step counts (good_steps: applied steps only) and after `interval` clean
    steps in a row the scale grows, unless the grown scale would not be finite: then it stays, and the tracker restarts all the same."""
    scale, tracker, found, good = (F32(x) for x in np.asarray(state, dtype=F32))
    growth, backoff = F32(growth), F32(backoff)
    if found != 0:
        scale, tracker = F32(scale * backoff), F32(0)
    else:
        good = F32(good + F32(1))
        tracker = F32(tracker + F32(1))
        if tracker >= F32(interval):
            with np.errstate(over="ignore"):
                grown = F32(scale * growth)
            if np.isfinite(grown):
                scale = grown
            tracker = F32(0)
    return np.array([scale, tracker, 0, good], dtype=F32)


# (name, initial state, growth, backoff, interval, events); an event is 'c' (clean step) or the non-finite value the step's gradients hold
SCALER_SCRIPTS = [
    # clean steps across two growth boundaries, inf / NaN / -inf steps, and a backoff directly after a growth
    ("mixed", [1024.0, 0, 0, 0], 2.0, 0.5, 4, ["c"] * 9 + ["inf", "nan", "c", "-inf"] + ["c"] * 4 + ["inf"] + ["c"] * 5 + ["nan"]),
    ("interval1", [4.0, 0, 0, 0], 2.0, 0.5, 1, ["c", "c", "inf", "c", "-inf", "nan", "c"]),
    ("backoff1", [256.0, 2, 0, 5], 1.5, 1.0, 4, ["inf", "c", "c", "c", "c", "nan", "c"]),
    # the grown scale is not finite: the scale stays 2^127, the tracker restarts, the step counts
    ("top", [2.0 ** 127, 3, 0, 7], 2.0, 0.5, 4, ["c", "c", "c", "c", "c", "inf", "c", "c", "c", "c"]),
]
EVENT_VALUE = {"inf": np.inf, "-inf": -np.inf, "nan": np.nan}


def run_scaler_script(script):
    """-> float32 [len(events), 4]: the state after every step"""
    _, state, growth, backoff, interval, events = script
    state = np.array(state, dtype=F32)
    out = []
    for e in events:
        if e != "c":
            state[2] = 1.0
        state = scaler_reference(state, growth, backoff, interval)
        out.append(state.copy())
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ data-parallel pack / reduce
def pack_reference(g, scale):
    """float16 round-to-nearest-even of the float32 product g * scale, on the bits: overflow to +-inf, subnormals and -0 kept, NaN -> a NaN
    (sign kept, payload 0x200: compare NaNs as NaNs, not by payload)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.ascontiguousarray(np.asarray(g, dtype=F32) * F32(scale), dtype=F32)
    b = x.view(np.uint32).astype(np.uint64)
    sign = (b >> np.uint64(16)) & np.uint64(0x8000)
    e = ((b >> np.uint64(23)) & np.uint64(0xFF)).astype(np.int64)
    man = b & np.uint64(0x7FFFFF)

    def rne(q, rem, half):
        return q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)

    # normal halves: exponent e - 112 in 1..30; a carry out of the mantissa walks into the exponent, and past 65504 into inf
    hn = rne(((np.maximum(e - 112, 0)).astype(np.uint64) << np.uint64(10)) | (man >> np.uint64(13)), man & np.uint64(0x1FFF), np.uint64(0x1000))
    hn = np.where(e - 112 >= 31, np.uint64(0x7C00), np.minimum(hn, np.uint64(0x7C00)))
    # subnormal halves (and what rounds up into the smallest normal): the 24-bit significand in units of 2^-24
    s = np.clip(126 - e, 14, 40).astype(np.uint64)
    full = man | np.uint64(0x800000)
    one = np.uint64(1)
    hs = rne(full >> s, full & ((one << s) - one), one << (s - one))
    hs = np.where(e == 0, np.uint64(0), hs)                   # float32 subnormals are far below half of 2^-24
    h = np.where(e - 112 >= 1, hn, hs)
    h = np.where(e == 255, np.where(man != 0, np.uint64(0x7E00), np.uint64(0x7C00)), h)
    return (sign | h).astype(np.uint16).view(np.float16).reshape(x.shape)


def reduce_reference(recv, world):
    """recv: float16 [world, shard] -> (the float32 sum of the slices in rank order, starting from +0; whether that sum holds a non-finite value).
    A float16 widens to float32 exactly and the adds are float32's own, so this is exact."""
    recv = np.asarray(recv)
    assert recv.dtype == np.float16 and recv.shape[0] == world
    acc = np.zeros(recv.shape[1], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(world):
            acc = (acc + recv[r].astype(F32)).astype(F32)
    return acc, bool(not np.isfinite(acc).all())


def half_edges():
    """float32 values at the edges of float16 -> (values, expected float16 bit patterns or None for NaN)"""
    above = np.nextafter(F32(2.0 ** -25), F32(1))
    edges = [(65504.0, 0x7BFF), (-65504.0, 0xFBFF), (65519.996, 0x7BFF), (65520.0, 0x7C00), (-65520.0, 0xFC00), (1e5, 0x7C00), (2.0 ** -14, 0x0400),
             (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (-(2.0 ** -25), 0x8000), (above, 0x0001), (3 * 2.0 ** -25, 0x0002), (5 * 2.0 ** -25, 0x0002),
             (-0.0, 0x8000), (0.0, 0x0000), (np.inf, 0x7C00), (-np.inf, 0xFC00), (np.nan, None),
             (2.0 ** -14 - 2.0 ** -25, 0x0400), (1.0 + 2.0 ** -11, 0x3C00), (1.0 + 3 * 2.0 ** -11, 0x3C02), (2047.5, 0x6800), (1e-30, 0x0000)]
    return np.array([e[0] for e in edges], dtype=F32), [e[1] for e in edges]


def same_halves(a, b):
    """bit for bit, NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float16), np.asarray(b, dtype=np.float16)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a.view(np.uint16)[~na] == b.view(np.uint16)[~nb]).all())
