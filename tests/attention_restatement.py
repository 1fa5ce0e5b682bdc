"""NumPy restatement of the fused attention of customnerf_amd/csrc/sd_attn.hip, and the inputs that pin it down.

Three things live here, shared by tests/test_sd_attention_host.py (CPU) and tests/test_gpu_sd_attention.py (GPU):

  * `reference`: softmax(q k^T / sqrt(d)) v per head in float64 from the fp16 input values, with the per-element weight spread
    S = sum_j w_j |v_j - ref| / sum_j w_j, and `tol`, the fixed bound  2^-10 (|ref| + S) + Tk 2^-24 max|v| + 2^-24:
    every probability is rounded once to fp16 (relative 2^-11) and the same rounded value enters numerator and denominator, so to
    first order the error is 2^-11 S; the fp16 result adds 2^-11 |ref|; the factor 2 covers the 1 ulp of v_exp_f32, the fp32
    accumulation and the second-order terms; the middle term covers probabilities flushed or denormalised below fp16's range.
  * `emulate`: what a correct kernel of this design computes — tile-wise online softmax with the running maximum in raw score units,
    `corr` per tile, probabilities rounded to fp16, fp32 accumulators, the denominator either as an fp32 sum of the rounded
    probabilities or as one more accumulated "ones" row, a final multiply by 1.0f / l and the fp16 rounding — written from the
    kernel's comments; `defect=` plants one of DEFECTS in it, which is how the host test shows that the probes have teeth.
    `emulate_fallback` is the explicit-scores path (fp16 scores, fp32 softmax, fp16 probabilities, fp32 product).
  * the input generators.  All values are fp16; each generator asserts its own preconditions.
      selector     every key carries a +-1 code (code bits repeated over all d channels: every k-step fragment takes part), q_i is a
                   power of two times the code of its target key, every other key trails by >= 40 bits: the output is V[target], bit
                   for bit.  Codes are pairwise distinct as far as 2^d allows (d = 8 has 256); what is asserted is what the probe
                   needs: the codes of the targets differ from every other key's code by the Hamming distance the amplitude is
                   derived from.
      uniform      the keys of a subset carry the query's code (p = 1 each), V holds non-zero integers in [-15, 15] (exact fp32 sums):
                   the output is the mean over the subset, at most 1 fp16 ulp from the float64 mean rounded to fp16.  Every channel has
                   one sign, so that no mean cancels: see uniform().
      trajectory   amplitude x shared direction + a small Gaussian part, with the row maximum ascending / descending / spiking /
                   climbing a staircase of > 150 bits per tile / constant and hugely negative / mixed within a wave; checked with `tol`.
      poison       K and V are the first Tk rows of buffers with 64 more rows, which hold NaN, or (K) the target's code at double
                   amplitude: one read past Tk changes the result.
      temptation   causal: every query's segment code sits, at double amplitude, in the keys of all later segments; the output is
                   still V[t(i)], t(i) <= i the last segment start (t(i) = i and t(i) = 0 included).
"""
import math

import numpy as np

LOG2E = 1.4426950408889634
GAP_BITS = 40.0                      # every non-selected key trails the selected one by this many bits: p < 2^-40 rounds to fp16 zero
MAX_BITS = 4096.0                    # |m * scale_log2e| below this: the fma's rounding of m * scale (2^-24 relative) keeps exp2 within fp16's 1.0
POISON_ROWS = 64
F16_MAX = 65504.0
DEFECTS = ("drop_last_key", "include_past_key", "swap_v_slots", "skip_rescale", "causal_ge", "next_head_v")

f16, f32, f64 = np.float16, np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ reference and bound
def reference(q, k, v, heads, causal=False):
    """-> (ref, spread), float64 [B, Tq, C]"""
    B, Tq, C = q.shape
    Tk, d = k.shape[1], C // heads
    ref, spread = np.empty((B, Tq, C), f64), np.empty((B, Tq, C), f64)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            Q, K, V = q[b, :, sl].astype(f64), k[b, :, sl].astype(f64), v[b, :, sl].astype(f64)
            s = Q @ K.T / math.sqrt(d)
            if causal:
                s = np.where(np.arange(Tk)[None, :] > np.arange(Tq)[:, None], -np.inf, s)
            w = np.exp(s - s.max(1, keepdims=True))
            w /= w.sum(1, keepdims=True)
            r = w @ V
            ref[b, :, sl] = r
            for i0 in range(0, Tq, 16):                           # in blocks of queries that stay in cache
                dev = V[None, :, :] - r[i0:i0 + 16, None, :]
                np.abs(dev, out=dev)
                spread[b, i0:i0 + 16, sl] = (w[i0:i0 + 16, None, :] @ dev)[:, 0, :]
    return ref, spread


def tol(ref, spread, v, Tk):
    return 2.0 ** -10 * (np.abs(ref) + spread) + Tk * 2.0 ** -24 * float(np.abs(v.astype(f64)).max()) + 2.0 ** -24


def err_over_tol(got, ref, spread, v, Tk):
    """largest |got - ref| / tol (inf when got is not finite)"""
    g = np.asarray(got, f64)
    if not np.isfinite(g).all():
        return math.inf
    return float((np.abs(g - ref) / tol(ref, spread, v, Tk)).max())


def ulp_distance(a, b):
    """distance in fp16 units in the last place between two fp16 arrays (finite values)"""
    def ordered(x):
        u = np.ascontiguousarray(x, f16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.abs(ordered(a) - ordered(b))


# ------------------------------------------------------------------------------------------------------------------ arithmetic model
def _exp2_f32(x):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(x.astype(f64)).astype(f32)


def _truncating_sum(acc, p, v):
    """acc + p v as a multi-operand adder that aligns its 17 addends to the largest one and drops the bits below 2^-24 of it (towards
    -inf) before it sums: a guess at the MFMA's adder that reproduces the one thing measured on an MI355X — a mean of exactly zero came out
    as -2^-23 (see uniform())"""
    terms = np.concatenate([acc[:, None, :].astype(f64), p[:, :, None] * v[None, :, :]], 1)
    mx = np.abs(terms).max(1)
    grid = 2.0 ** (np.floor(np.log2(np.where(mx > 0, mx, 1.0))) - 24.0)
    return (np.floor(terms / grid[:, None, :]) * grid[:, None, :]).sum(1).astype(f32)


def emulate(q, k, v, heads, causal=False, keys_per_iter=32, ones_channel=False, defect=None, tk=None, adder="exact"):
    """The fused kernel's arithmetic.  k / v may hold rows past the `tk` valid ones (memory behind the problem): only a defect reads them.
    adder: "exact" (every k-step's sum rounded once) or "truncating" (_truncating_sum)."""
    assert defect is None or defect in DEFECTS
    B, Tq, C = q.shape
    Tk = k.shape[1] if tk is None else tk
    d, KEYS = C // heads, keys_per_iter
    c = f32(f32(LOG2E) / np.sqrt(f32(d)))
    n_t = (Tk + KEYS - 1) // KEYS
    rows = n_t * KEYS + KEYS
    out = np.empty((B, Tq, C), f16)
    qi = np.arange(Tq)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for b in range(B):
            for h in range(heads):
                hv = (h + 1) % heads if defect == "next_head_v" else h
                Q = q[b, :, h * d:(h + 1) * d].astype(f64)
                K = np.zeros((rows, d), f64)
                V = np.zeros((rows, d), f64)
                K[:min(k.shape[1], rows)] = k[b, :rows, h * d:(h + 1) * d]
                V[:min(v.shape[1], rows)] = v[b, :rows, hv * d:(hv + 1) * d]
                S = np.zeros((Tq, rows), f32)                   # one rounding per MFMA k-step of 16 channels (products of fp16 values are exact)
                for c0 in range(0, d, 16):
                    S = (S + Q[:, c0:c0 + 16] @ K[:, c0:c0 + 16].T).astype(f32)
                m = np.full(Tq, -np.inf, f32)
                l = np.zeros(Tq, f32)
                o = np.zeros((Tq, d), f32)
                skipped = False
                for t in range(n_t):
                    key = np.arange(t * KEYS, (t + 1) * KEYS)
                    valid = key < Tk
                    partial = t * KEYS < Tk < (t + 1) * KEYS
                    if defect == "drop_last_key" and partial:
                        valid[Tk - 1 - t * KEYS] = False
                    if defect == "include_past_key" and partial:
                        valid[Tk - t * KEYS] = True
                    mask = np.broadcast_to(valid[None, :], (Tq, KEYS))
                    if causal:
                        future = key[None, :] >= qi[:, None] if defect == "causal_ge" else key[None, :] > qi[:, None]
                        mask = mask & ~future
                    s = np.where(mask, S[:, key], f32(-np.inf))
                    m_new = np.maximum(np.maximum(m, s.max(1)), f32(-1e30))
                    moved = m_new != m
                    corr = np.where(moved, _exp2_f32((m - m_new) * c), f32(1.0))
                    if defect == "skip_rescale" and t > 0 and not skipped and moved.any():
                        corr, skipped = np.ones(Tq, f32), True
                    m = m_new
                    nm = (-m_new * c).astype(f32)
                    arg = (s.astype(f64) * f64(c) + nm.astype(f64)[:, None]).astype(f32)          # fused multiply-add: one rounding
                    ph = _exp2_f32(arg).astype(f16)
                    o = (o * corr[:, None]).astype(f32)
                    l = (l * corr).astype(f32)
                    if not ones_channel:
                        l = (l + ph.astype(f64).sum(1).astype(f32)).astype(f32)
                    vkey = key.copy()
                    if defect == "swap_v_slots" and t == 0:
                        vkey[0], vkey[1] = key[1], key[0]
                    for g in range(KEYS // 16):                  # one MFMA k-step: 16 keys
                        grp = slice(16 * g, 16 * g + 16)
                        pg = ph[:, grp].astype(f64)
                        live = (vkey[grp] < Tk) | (valid[grp] & (vkey[grp] == key[grp]))     # rows behind the problem are staged as zeros, not read
                        if adder == "truncating":
                            o = _truncating_sum(o, pg[:, live], V[vkey[grp][live]])
                        else:
                            o = (o + pg[:, live] @ V[vkey[grp][live]]).astype(f32)
                        if ones_channel:
                            l = (l + pg.sum(1)).astype(f32)
                inv = (f32(1.0) / l).astype(f32)
                out[b, :, h * d:(h + 1) * d] = (o * inv[:, None]).astype(f32).astype(f16)
    return out


def emulate_fallback(q, k, v, heads):
    """The explicit-scores path of ops.attention (d > 160 or d % 8): fp16 scores, fp32 softmax, fp16 probabilities, fp32 product."""
    B, Tq, C = q.shape
    d = C // heads
    alpha = f32(1.0 / float(d) ** 0.5)
    out = np.empty((B, Tq, C), f16)
    with np.errstate(over="ignore", under="ignore"):
        for b in range(B):
            for h in range(heads):
                sl = slice(h * d, (h + 1) * d)
                S = ((q[b, :, sl].astype(f64) @ k[b, :, sl].astype(f64).T).astype(f32) * alpha).astype(f16).astype(f32)
                e = np.exp((S - S.max(1, keepdims=True)).astype(f64)).astype(f32)
                inv = (f32(1.0) / e.astype(f64).sum(1).astype(f32)).astype(f32)
                P = (e * inv[:, None]).astype(f16)
                out[b, :, sl] = (P.astype(f64) @ v[b, :, sl].astype(f64)).astype(f32).astype(f16)
    return out


# ------------------------------------------------------------------------------------------------------------------ codes and amplitudes
def _rng(*key):
    return np.random.default_rng([int(x) for x in key])


def _tile_bits(bits, d):
    """[n, nb] bits -> [n, d] +-1, code bits repeated over the d channels"""
    nb = bits.shape[1]
    return (2.0 * bits[:, np.arange(d) % nb] - 1.0).astype(f64)


def make_codes(n_special, n_other, d, rng):
    """-> (special [n_special, d], other [n_other, d], hmin): +-1 codes; the special ones differ from every other code (special or not) in at
    least hmin >= 1 channels.  All codes are pairwise distinct when 2^min(d, 16) allows, else the non-special ones repeat."""
    nb = min(d, 16)
    total = 1 << nb
    assert n_special <= total - (1 if n_other else 0), "more selected keys than distinct codes"
    ids = rng.choice(total, min(total, n_special + n_other), replace=False)
    sp = ids[:n_special]
    rest = ids[n_special:]
    if n_other:
        assert len(rest) > 0
        ot = rest[np.arange(n_other) % len(rest)]
    else:
        ot = rest[:0]
    def expand(i):
        return _tile_bits(((i[:, None] >> np.arange(nb)[None, :]) & 1).astype(f64), d)
    S, O = expand(sp), expand(ot)
    hmin = d
    if n_special:
        allc = np.concatenate([S, O])
        dist = (d - S @ allc.T) / 2.0                            # Hamming distance over the d channels
        dist[np.arange(n_special), np.arange(n_special)] = d
        hmin = int(dist.min())
    assert hmin >= 1
    return S, O, hmin


def amplitude(d, hmin_dot, score_type="f32", norm2=None):
    """smallest power of two A such that a key whose dot product with the query's unit-amplitude code trails the selected key's by
    `hmin_dot` trails by >= GAP_BITS bits after the 1/sqrt(d) scale — in `score_type` (the fallback rounds its scores to fp16)."""
    norm2 = d if norm2 is None else norm2
    A = 1.0
    while True:
        top = A * norm2 / math.sqrt(d)
        gap = A * hmin_dot / math.sqrt(d)
        if score_type == "f16":
            gap -= 2.0 * float(np.spacing(f16(top)))             # both scores rounded to fp16
        if gap * LOG2E >= GAP_BITS:
            break
        A *= 2.0
    assert top * LOG2E * 2.0 < MAX_BITS, "amplitude leaves the range in which p = 1 is exact"
    assert 2.0 * top < (F16_MAX if score_type == "f16" else 3e38) and 2.0 * A <= F16_MAX
    return A


def _v_distinct(B, Tk, heads, d, rng):
    """rows with |v| in [1/4, 4), pairwise distinct within every head (and across heads)"""
    mant = 1.0 + rng.integers(0, 1024, (B, Tk, heads * d)) / 1024.0
    v = (mant * 2.0 ** rng.integers(-2, 2, mant.shape) * rng.choice([-1.0, 1.0], mant.shape)).astype(f16)
    a = np.abs(v.astype(f64))
    assert (a >= 0.25).all() and (a < 4.0).all()
    w = rng.standard_normal(d)
    for b in range(B):                                            # rows whose projections on one direction differ are different rows
        proj = np.concatenate([v[b, :, h * d:(h + 1) * d].astype(f64) @ w for h in range(heads)])
        assert len(np.unique(proj)) == len(proj), "V rows are not distinct"
    return v


def _as16(x):
    y = x.astype(f16)
    assert np.isfinite(y.astype(f64)).all()
    return y


class Probe:
    """one input set: q, k, v (fp16, [B, T, C]), and what the check needs"""
    def __init__(self, name, q, k, v, heads, causal=False, expect=None, k_buf=None, v_buf=None):
        self.name, self.q, self.k, self.v, self.heads, self.causal, self.expect = name, q, k, v, heads, causal, expect
        self.k_buf, self.v_buf = k_buf, v_buf                    # poison: the buffers k and v are the leading rows of


# ------------------------------------------------------------------------------------------------------------------ selector
SELECTOR_MAPS = ("perm", "first", "last", "slots", "per_head")


def selector_targets(kind, B, heads, Tq, Tk, causal, rng):
    """-> target key of every query, int [B, heads, Tq]"""
    i = np.arange(Tq)
    n = (np.arange(B * heads)[:, None] * Tq + i[None, :]).reshape(B, heads, Tq)
    if kind == "first":
        t = np.zeros((B, heads, Tq), np.int64)
    elif kind == "last":
        t = np.broadcast_to(i if causal else np.full(Tq, Tk - 1), (B, heads, Tq)).copy()
    elif kind == "perm":
        p = rng.permutation(Tk)
        t = np.broadcast_to(p[i % Tk], (B, heads, Tq)).copy()
    elif kind == "slots":                                         # key = 33 n (34 n where 33 shares a factor with Tk): the next tile and the next slot with every query
        step = 33 if math.gcd(33, Tk) == 1 else 34
        assert math.gcd(step, Tk) == 1
        t = (step * n) % Tk
        if B * heads * Tq >= Tk:                                  # then every key, so every slot of every tile, is somebody's target
            assert len(np.unique(t)) == Tk
    elif kind == "per_head":                                      # a different map per head and per batch entry
        t = np.stack([rng.permutation(max(Tk, Tq))[:Tq] % Tk for _ in range(B * heads)]).reshape(B, heads, Tq)
        if B * heads > 1 and Tk > 8 and Tq > 4:
            assert any((t[0, 0] != t.reshape(-1, Tq)[j]).any() for j in range(1, B * heads))
    else:
        raise ValueError(kind)
    if causal:
        t = np.minimum(t, i[None, None, :]) if kind != "perm" else t % (i[None, None, :] + 1)
    assert (t >= 0).all() and (t < Tk).all() and (not causal or (t <= i).all())
    return t


def selector(kind, B, heads, Tq, Tk, d, causal=False, score_type="f32", seed=0):
    rng = _rng(1, SELECTOR_MAPS.index(kind), B, heads, Tq, Tk, d, int(causal), seed)
    t = selector_targets(kind, B, heads, Tq, Tk, causal, rng)
    C = heads * d
    q, k = np.zeros((B, Tq, C), f64), np.zeros((B, Tk, C), f64)
    v = _v_distinct(B, Tk, heads, d, rng)
    expect = np.empty((B, Tq, C), f16)
    for b in range(B):
        for h in range(heads):
            sel = np.unique(t[b, h])
            S, O, hmin = make_codes(len(sel), Tk - len(sel), d, rng)
            A = amplitude(d, 2 * hmin, score_type)
            codes = np.empty((Tk, d))
            codes[sel] = S
            codes[np.setdiff1d(np.arange(Tk), sel)] = O
            sl = slice(h * d, (h + 1) * d)
            k[b, :, sl] = codes
            q[b, :, sl] = A * codes[t[b, h]]
            expect[b, :, sl] = v[b, t[b, h], sl]
            # precondition, in float64: every other key trails the target by >= GAP_BITS bits
            s = (q[b, :, sl] @ codes.T) / math.sqrt(d) * LOG2E
            top = s[np.arange(Tq), t[b, h]]
            s[np.arange(Tq), t[b, h]] = -np.inf
            if causal:
                s = np.where(np.arange(Tk)[None, :] > np.arange(Tq)[:, None], -np.inf, s)
            assert Tk == 1 or (top - s.max(1) >= GAP_BITS - 1e-9).all()
    return Probe(f"selector/{kind}", _as16(q), _as16(k), v, heads, causal, expect)


# ------------------------------------------------------------------------------------------------------------------ uniform subset
UNIFORM_KINDS = ("all", "per_tile", "straddle", "last_tile", "sizes")


def uniform_subsets(kind, Tk, rng):
    """-> list of disjoint key subsets"""
    n_t = (Tk + 31) // 32
    if kind == "all":
        subs = [np.arange(Tk)]
    elif kind == "per_tile":                                      # one key per 32-key tile, two different slot patterns
        subs = []
        for off in (3, 20):
            s = np.array([min(32 * t + (7 * t + off) % 32, Tk - 1) for t in range(n_t)])
            subs.append(np.unique(s))
        subs[1] = np.setdiff1d(subs[1], subs[0])
    elif kind == "straddle":                                      # two keys on either side of every 32-key boundary
        subs = [np.arange(max(b0 - 2, 0), min(b0 + 2, Tk)) for b0 in range(32, Tk, 32)] or [np.arange(Tk)]
    elif kind == "last_tile":                                     # only the (partial) last tile
        subs = [np.arange(32 * (n_t - 1), Tk)]
    elif kind == "sizes":                                         # powers of two and not
        p, subs, at = rng.permutation(Tk), [], 0
        for n in (1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 32, 33):
            if at + n > Tk:
                break
            subs.append(np.sort(p[at:at + n]))
            at += n
    else:
        raise ValueError(kind)
    subs = [s for s in subs if len(s)]
    allk = np.concatenate(subs)
    assert len(subs) and len(np.unique(allk)) == len(allk) and allk.min() >= 0 and allk.max() < Tk
    return subs


def uniform(kind, B, heads, Tq, Tk, d, causal=False, score_type="f32", seed=0, cancelling=False):
    """V's integers carry one sign per channel (half the channels negative), so |mean| >= 1.  With a sign per element (`cancelling`) a mean
    can be exactly zero, and there "within 1 ulp" asks for an exact zero, which the hardware does not give: the accumulator still holds
    what the keys before the subset left, scaled by corr <= 2^-40, and the MFMA's adder turned that negligible negative rest into -2^-21
    next to addends of 8 — measured on an MI355X as -2^-23 for a mean of 0 over four keys, in the LDS-DMA and the register-staged kernels alike.  That is fp32
    accumulation error (2^-24 of the largest addend), not a lost key; tests/test_sd_attention_host.py reproduces both sides with
    emulate(adder="truncating")."""
    rng = _rng(2, UNIFORM_KINDS.index(kind), B, heads, Tq, Tk, d, int(causal), seed)
    C = heads * d
    q, k = np.zeros((B, Tq, C), f64), np.zeros((B, Tk, C), f64)
    mag = rng.integers(1, 16, (B, Tk, C))
    sign = rng.choice([-1, 1], (B, Tk, C)) if cancelling else np.where(rng.permutation(C) % 2 == 0, 1, -1)[None, None, :]
    v = (mag * sign).astype(f16)
    expect = np.empty((B, Tq, C), f16)
    for b in range(B):
        for h in range(heads):
            subs = uniform_subsets(kind, Tk, rng)
            if causal:                                            # key 0 alone is the subset of the queries no other subset lies behind
                subs = [np.array([0])] + [s[s != 0] for s in subs]
                subs = [s for s in subs if len(s)]
            member = np.concatenate(subs)
            S, O, hmin = make_codes(len(subs), Tk - len(member), d, rng)
            A = amplitude(d, 2 * hmin, score_type)
            codes = np.empty((Tk, d))
            for g, s in enumerate(subs):
                codes[s] = S[g]
            codes[np.setdiff1d(np.arange(Tk), member)] = O
            sl = slice(h * d, (h + 1) * d)
            k[b, :, sl] = codes
            last = np.array([s.max() for s in subs])
            means = np.stack([v[b, s, sl].astype(f64).mean(0) for s in subs])
            assert cancelling or (np.abs(means) >= 1.0).all()
            s64 = (A * S) @ codes.T / math.sqrt(d) * LOG2E        # per subset: its keys tie, every other key (visible or not) trails
            for g, sub in enumerate(subs):
                inside = np.zeros(Tk, bool)
                inside[sub] = True
                assert (s64[g, inside] == s64[g, sub[0]]).all()
                assert inside.all() or s64[g, sub[0]] - s64[g, ~inside].max() >= GAP_BITS - 1e-9
            i = np.arange(Tq)
            if causal:                                            # round-robin over the subsets that lie wholly at or before the query
                order = np.argsort(last, kind="stable")
                n_ok = np.searchsorted(last[order], i, side="right")
                assert (n_ok >= 1).all()
                gi = order[(i + b + h) % n_ok]
                assert (last[gi] <= i).all()
            else:
                gi = (i + b + h) % len(subs)
            q[b, :, sl] = A * S[gi]
            expect[b, :, sl] = means[gi].astype(f16)
    assert (np.abs(v.astype(f64)) >= 1).all() and (np.abs(v.astype(f64)) <= 15).all()
    return Probe(f"uniform/{kind}", _as16(q), _as16(k), v, heads, causal, expect)


# ------------------------------------------------------------------------------------------------------------------ trajectories
TRAJECTORY_KINDS = ("ascending", "descending", "spike", "staircase", "equal_negative", "mixed")
STAIR_BITS = 170.0                   # nominal rise per 32-key tile of the staircase (asserted: > 150 bits for every query)


def trajectory(kind, B, heads, Tq, Tk, d, causal=False, seed=0):
    rng = _rng(3, TRAJECTORY_KINDS.index(kind), B, heads, Tq, Tk, d, int(causal), seed)
    C = heads * d
    v = _as16(rng.standard_normal((B, Tk, C)))
    j = np.arange(Tk)
    if kind == "equal_negative":                                  # raw q . k around -3e4, the same for every key
        kv = float(f16(round(3.0e4 / (16.0 * d))))
        q, k = np.full((B, Tq, C), 16.0), np.full((B, Tk, C), -kv)
        raw = -16.0 * kv * d
        assert -3.3e4 < raw < -2.7e4
        return Probe(f"trajectory/{kind}", _as16(q), _as16(k), v, heads, causal)
    span = 12.0
    ramp = span * j / max(Tk - 1, 1)
    sign = np.ones(Tq)
    if kind == "ascending":
        prof = ramp.copy()
        prof[-1] += 4.0
    elif kind == "descending":
        prof = -ramp
        prof[0] += 4.0
    elif kind == "spike":
        prof = np.zeros(Tk)
        prof[min(32 * (((Tk + 31) // 32) // 2) + 13, Tk - 1)] = 8.0
    elif kind == "staircase":
        prof = STAIR_BITS / LOG2E * (j // 32)
    elif kind == "mixed":                                         # odd queries ascend, even queries descend: lanes of one wave disagree
        prof = ramp
        sign = np.where(np.arange(Tq) % 2 == 1, 1.0, -1.0)
    else:
        raise ValueError(kind)
    sq, sk = (0.03, 0.5) if kind == "staircase" else (0.125, 0.5)
    q, k = np.empty((B, Tq, C)), np.empty((B, Tk, C))
    for b in range(B):
        for h in range(heads):
            u = rng.choice([-1.0, 1.0], d)
            sl = slice(h * d, (h + 1) * d)
            q[b, :, sl] = sign[:, None] * u[None, :] + sq * rng.standard_normal((Tq, d))
            k[b, :, sl] = (prof / math.sqrt(d))[:, None] * u[None, :] + sk * rng.standard_normal((Tk, d))
    q, k = _as16(q), _as16(k)
    for b in range(B):                                            # preconditions on the fp16 values, in float64
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = q[b, :, sl].astype(f64) @ k[b, :, sl].astype(f64).T / math.sqrt(d)
            assert (np.abs(s) * LOG2E < MAX_BITS).all()
            if causal:
                continue
            w = np.exp(s - s.max(1, keepdims=True))
            w /= w.sum(1, keepdims=True)
            am = s.argmax(1)
            if kind == "ascending":
                assert (am == Tk - 1).mean() >= 0.9
            elif kind == "descending":
                assert (am == 0).mean() >= 0.9
            elif kind == "mixed" and Tk > 64:
                assert (am[1::2] > Tk / 2).all() and (am[0::2] < Tk / 2).all()
            elif kind == "staircase":
                tmax = np.array([s[:, a:a + 32].max(1) for a in range(0, Tk, 32)])
                assert len(tmax) == 1 or (np.diff(tmax, axis=0) * LOG2E > 150.0).all()
            if kind != "staircase" and Tk >= 33:
                assert w.max(1).mean() < 0.999, "rows are one-hot"
                assert (w.max(1) > 2.0 / Tk).all(), "rows are flat"
    return Probe(f"trajectory/{kind}", q, k, v, heads, causal)


# ------------------------------------------------------------------------------------------------------------------ poison
POISON_KINDS = ("nan", "tempt")


def poison(kind, B, heads, Tq, Tk, d, causal=False, score_type="f32", seed=0):
    """A selector whose K and V are the leading Tk rows of buffers with POISON_ROWS more rows.  'nan': those rows are NaN in K and V;
    'tempt' (B = 1, so that the rows lie directly behind the valid ones): all queries select the last valid key and the K rows behind it
    hold that key's code at double amplitude, the V rows NaN."""
    if kind == "tempt":
        assert B == 1
    base = selector("last" if kind == "tempt" else "perm", B, heads, Tq, Tk, d, causal, score_type, seed=seed + 17)
    C = heads * d
    kb = np.full((B, Tk + POISON_ROWS, C), np.nan, f16)
    vb = np.full((B, Tk + POISON_ROWS, C), np.nan, f16)
    kb[:, :Tk], vb[:, :Tk] = base.k, base.v
    if kind == "tempt":
        if causal:                                                # the last query's key: the one the rows behind Tk would beat
            kb[:, Tk:] = 2.0 * base.k[:, Tq - 1:Tq].astype(f64)
        else:
            kb[:, Tk:] = 2.0 * base.k[:, Tk - 1:Tk].astype(f64)
        assert np.isfinite(kb.astype(f64)).all()
    return Probe(f"poison/{kind}", base.q, kb[:, :Tk], vb[:, :Tk], heads, causal, base.expect, k_buf=kb, v_buf=vb)


# ------------------------------------------------------------------------------------------------------------------ causal temptation
def temptation_starts(T, nseg):
    cand = [c for c in (0, 1, 31, 32, 33, 63, 64, 65, T // 2, 127, 128, 129, T - 2, T - 1) if 0 <= c < T]
    cand = sorted(set(cand))
    if len(cand) > nseg:                                          # keep 0 and T - 1, spread the rest
        idx = np.unique(np.round(np.linspace(0, len(cand) - 1, nseg)).astype(int))
        cand = [cand[i] for i in idx]
    return np.array(cand)


def temptation(B, heads, T, d, seed=0):
    """Causal, Tq = Tk = T.  Segment s starts at key r_s and owns the channels c % nseg == s, where its code c_s lives.  Key r_s carries
    c_s; every key of a later segment carries 2 c_s.  A query of segment s is A c_s: among the keys <= i only r_s answers; every key of
    a later segment — all of them > i — answers twice as loud."""
    rng = _rng(4, B, heads, T, d, seed)
    C = heads * d
    nseg = min(8, d // 2)
    starts = temptation_starts(T, nseg)
    seg = np.searchsorted(starts, np.arange(T), side="right") - 1
    assert starts[0] == 0 and (seg >= 0).all()
    t = starts[seg]
    assert (t <= np.arange(T)).all() and t[0] == 0 and (t == np.arange(T)).any()
    supp = np.array([(np.arange(d) % nseg == s).sum() for s in range(len(starts))])
    A = amplitude(d, float(supp.min()), norm2=float(2 * supp.max()))
    q, k = np.zeros((B, T, C)), np.zeros((B, T, C))
    v = _v_distinct(B, T, heads, d, rng)
    expect = np.empty((B, T, C), f16)
    for b in range(B):
        for h in range(heads):
            codes = np.zeros((len(starts), d))
            for s in range(len(starts)):
                ch = np.arange(d) % nseg == s
                codes[s, ch] = rng.choice([-1.0, 1.0], ch.sum())
            earlier = np.cumsum(codes, 0) - codes                 # sum of the codes of the segments before s
            kk = 2.0 * earlier[seg]
            kk[starts] += codes
            sl = slice(h * d, (h + 1) * d)
            k[b, :, sl] = kk
            q[b, :, sl] = A * codes[seg]
            expect[b, :, sl] = v[b, t, sl]
            s64 = q[b, :, sl] @ kk.T / math.sqrt(d) * LOG2E
            i = np.arange(T)
            top = s64[i, t]
            past = np.where((i[None, :] <= i[:, None]) & (i[None, :] != t[:, None]), s64, -np.inf)
            assert T == 1 or (top - past.max(1) >= GAP_BITS - 1e-9).all()
            fut = i[None, :] >= np.append(starts, T)[seg + 1][:, None]          # the keys of later segments
            assert (np.where(fut, s64, np.inf) >= 2.0 * top[:, None] - 1e-9).all()
    return Probe("temptation", _as16(q), _as16(k), v, heads, True, expect)


# ------------------------------------------------------------------------------------------------------------------ the GPU matrix
SHAPES = [(1, 1, 1, 1), (1, 1, 31, 33), (2, 2, 33, 63), (1, 3, 130, 65), (2, 4, 130, 129), (1, 1, 64, 193), (1, 2, 5, 333), (1, 1, 128, 64)]
CAUSAL_T = [1, 33, 77, 130, 200]
CAUSAL_SHAPES = [(1, 2, T, T) for T in CAUSAL_T]
DMA_DIMS = [40, 64, 80, 160]                                     # k_sd_attention_dma<D, KT> through ops.attention, <KS, DT, KT, false> through attention_vt
STAGED_DIMS = [8, 32, 48, 56, 96, 128]                           # k_sd_attention<3,2,2>, <4,2,2>, <5,3,1>, <10,5,1>, VROW
FUSED_DIMS = DMA_DIMS + STAGED_DIMS
FALLBACK_CASES = [(512, 1), (20, None)]                          # (head dim, heads: None = the shape's own)


def kernel_model(d):
    """(keys per iteration, ones channel) of the instantiation at_launch picks for head dim d"""
    ks, dt = (d + 15) // 16, (d + 31) // 32
    if d in (40, 64):
        kpi = 64
    elif d in (80, 160):
        kpi = 32
    else:
        kpi = 64 if (ks <= 4 and dt <= 2) else 32
    return kpi, d < 32 * dt


def _build(jobs):
    return [j[0](*j[1:]) for j in jobs]


def exact_probes(B, heads, Tq, Tk, d, causal, score_type="f32"):
    """the probes whose result is known exactly (selector, poison, temptation: bit-equal; uniform: <= 1 ulp)"""
    jobs = [(selector, kind, B, heads, Tq, Tk, d, causal, score_type) for kind in SELECTOR_MAPS]
    jobs += [(uniform, kind, B, heads, Tq, Tk, d, causal, score_type) for kind in UNIFORM_KINDS]
    jobs += [(poison, "nan", B, heads, Tq, Tk, d, causal, score_type), (poison, "tempt", 1, heads, Tq, Tk, d, causal, score_type)]
    if causal:
        jobs.append((temptation, B, heads, Tq, d))
    return _build(jobs)


def trajectory_probes(B, heads, Tq, Tk, d, causal):
    return _build([(trajectory, kind, B, heads, Tq, Tk, d, causal) for kind in TRAJECTORY_KINDS])


def references(probes):
    """-> [(ref, spread)] of reference() for every probe"""
    return _build([(reference, p.q, p.k, p.v, p.heads, p.causal) for p in probes])


def check_exact(p, got):
    """-> None if `got` (fp16 [B, Tq, C]) passes probe p's check, else a message"""
    got = np.asarray(got)
    if not np.isfinite(got.astype(f64)).all():
        return f"{p.name}: non-finite output"
    if p.name.startswith("uniform"):
        u = ulp_distance(got, p.expect)
        return None if u.max() <= 1 else f"{p.name}: {int(u.max())} ulp from the mean ({int((u > 1).sum())} elements)"
    bad = got.view(np.uint16) != p.expect.view(np.uint16)
    if bad.any():
        b, i, c = np.argwhere(bad)[0]
        return f"{p.name}: {int(bad.sum())} elements differ, first at [b {b}, query {i}, channel {c}]: {got[b, i, c]} for {p.expect[b, i, c]}"
    return None
