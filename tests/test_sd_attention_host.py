"""CPU: the probes of tests/test_gpu_sd_attention.py are sound and have teeth (tests/attention_restatement.py).

  * `reference` is softmax(q k^T / sqrt(d)) v: it agrees with torch's float64 scaled_dot_product_attention to 1e-12;
  * every generator's preconditions (asserted inside the generators) hold at every shape and head dim of the GPU matrix;
  * `emulate`, the arithmetic a correct kernel of this design performs, passes every check the GPU test applies, at 32 and 64 keys per
    iteration and with either form of the denominator: selector, poison and temptation bit-equal, uniform within 1 ulp, trajectories
    within `tol`.  Largest err / tol of the trajectories over the whole matrix, as printed by
    test_emulation_passes_every_gpu_check: 0.489 (spike; ascending 0.463, descending 0.471, staircase 0.460, equal_negative 0.485,
    mixed 0.423);
  * the uniform probes hold with an adder that truncates instead of rounding, which is what an MI355X has; values that may cancel do not;
  * each seeded defect of `emulate` fails at least one probe family at every shape where it can act.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))          # the sibling library
import attention_restatement as ar      # noqa: E402

ALL_SHAPES = [(s, False) for s in ar.SHAPES] + [(s, True) for s in ar.CAUSAL_SHAPES]
IDS = ["x".join(map(str, s)) + ("-causal" if c else "") for s, c in ALL_SHAPES]
MODELS = [(32, False), (32, True), (64, False), (64, True)]
EMULATED_DIMS = [8, 40, 64, 160]        # the arithmetic does not depend on d beyond the number of k-steps: the smallest, the largest, one of each denominator form


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,heads,Tq,Tk,d", [(2, 3, 37, 70, 24), (1, 2, 65, 65, 40), (1, 1, 1, 1, 8)])
def test_reference_is_sdpa(B, heads, Tq, Tk, d, causal):
    if causal:
        Tk = Tq
    g = np.random.default_rng(Tq + d)
    q, k, v = (g.standard_normal((B, T, heads * d)).astype(np.float16) for T in (Tq, Tk, Tk))
    ref, spread = ar.reference(q, k, v, heads, causal)
    qh, kh, vh = (torch.from_numpy(t.astype(np.float64)).view(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    want = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, is_causal=causal).transpose(1, 2).reshape(B, Tq, heads * d).numpy()
    assert np.abs(ref - want).max() <= 1e-12
    assert (spread >= 0).all() and np.isfinite(spread).all()


@pytest.mark.parametrize("shape,causal", ALL_SHAPES, ids=IDS)
def test_generator_preconditions_hold_over_the_gpu_matrix(shape, causal):
    """building a probe runs its generator's assertions; here also: fp16 values, shapes, and the expected value of every exact probe"""
    B, heads, Tq, Tk = shape
    cases = [(d, heads, "f32") for d in ar.FUSED_DIMS]
    if not causal:
        cases += [(d, heads if hh is None else hh, "f16") for d, hh in ar.FALLBACK_CASES]
    for d, hh, score_type in cases:
        probes = ar.exact_probes(B, hh, Tq, Tk, d, causal, score_type)
        if score_type == "f32":
            probes += ar.trajectory_probes(B, hh, Tq, Tk, d, causal)
        for p in probes:
            Bp = p.q.shape[0]
            assert p.q.dtype == p.k.dtype == p.v.dtype == np.float16
            assert p.q.shape == (Bp, Tq, hh * d) and p.k.shape == p.v.shape == (Bp, Tk, hh * d)
            assert np.isfinite(p.q.astype(np.float64)).all() and np.isfinite(p.k.astype(np.float64)).all()
            if p.expect is not None and not p.name.startswith("uniform"):
                ref, _ = ar.reference(p.q, p.k, p.v, hh, causal)                 # float64 agrees: the expected row carries all the weight
                assert np.abs(ref - p.expect.astype(np.float64)).max() <= 2.0 ** -36 * 4.0 * Tk
            if p.k_buf is not None:
                assert p.k_buf.shape[1] == Tk + ar.POISON_ROWS and np.shares_memory(p.k, p.k_buf) and np.shares_memory(p.v, p.v_buf)
                assert np.isnan(p.v_buf[:, Tk:].astype(np.float64)).all()


def _run(p, kpi, ones, defect=None):
    if p.k_buf is not None:
        return ar.emulate(p.q, p.k_buf, p.v_buf, p.heads, p.causal, kpi, ones, defect, tk=p.k.shape[1])
    return ar.emulate(p.q, p.k, p.v, p.heads, p.causal, kpi, ones, defect)


WORST = {}


@pytest.mark.parametrize("shape,causal", ALL_SHAPES, ids=IDS)
def test_emulation_passes_every_gpu_check(shape, causal):
    B, heads, Tq, Tk = shape
    worst = {}
    for d in EMULATED_DIMS:
        exact = ar.exact_probes(B, heads, Tq, Tk, d, causal)
        traj = ar.trajectory_probes(B, heads, Tq, Tk, d, causal)
        traj = list(zip(traj, ar.references(traj)))
        for kpi, ones in MODELS:
            for p in exact:
                msg = ar.check_exact(p, _run(p, kpi, ones))
                assert msg is None, (d, kpi, ones, msg)
            for p, (ref, spread) in traj:
                r = ar.err_over_tol(_run(p, kpi, ones), ref, spread, p.v, Tk)
                worst[p.name] = max(worst.get(p.name, 0.0), r)
                assert r < 1.0, (d, kpi, ones, p.name, r)
    for n, r in worst.items():
        WORST[n] = max(WORST.get(n, 0.0), r)
    print(f"[{'x'.join(map(str, shape))}{' causal' if causal else ''}] largest err / tol: " + ", ".join(f"{n.split('/')[1]} {r:.3f}" for n, r in worst.items()))
    print("    so far over the matrix: " + ", ".join(f"{n.split('/')[1]} {r:.3f}" for n, r in WORST.items()))


@pytest.mark.parametrize("shape", ar.SHAPES, ids=IDS[:len(ar.SHAPES)])
def test_fallback_model_passes_the_exact_probes(shape):
    """the explicit-scores path: fp16 scores hold the amplitudes its probes use, and the fp16 probability 1 / n (2^-11 off where n is no power
    of two) still leaves the uniform probes within 1 ulp: the products p v are exact in fp32 whatever the order of the sum"""
    B, heads, Tq, Tk = shape
    for d, hh in ar.FALLBACK_CASES:
        hh = heads if hh is None else hh
        for p in ar.exact_probes(B, hh, Tq, Tk, d, False, "f16"):
            msg = ar.check_exact(p, ar.emulate_fallback(p.q, p.k, p.v, hh))
            assert msg is None, (d, msg)


@pytest.mark.parametrize("shape,causal", ALL_SHAPES, ids=IDS)
def test_uniform_probes_do_not_depend_on_an_exact_adder(shape, causal):
    """with an adder that truncates below 2^-24 of its largest addend the uniform probes stay within 1 ulp ..."""
    B, heads, Tq, Tk = shape
    for d in (8, 64):
        kpi, ones = ar.kernel_model(d)
        for kind in ar.UNIFORM_KINDS:
            p = ar.uniform(kind, B, heads, Tq, Tk, d, causal)
            msg = ar.check_exact(p, ar.emulate(p.q, p.k, p.v, heads, causal, kpi, ones, adder="truncating"))
            assert msg is None, (d, msg)


@pytest.mark.parametrize("shape,d", [((1, 2, 5, 333), 8), ((2, 4, 130, 129), 32)])
def test_cancelling_values_would_ask_for_an_exact_adder(shape, d):
    """... whereas integers of either sign in one channel, whose mean can be exactly zero, pass with exact sums and fail with the truncating
    adder — at these two shapes in as many elements, and by as many ulp, as on an MI355X (1 element by 2 ulp, 65 elements by 3 ulp; -2^-23
    where the mean of four keys is 0): the reason for one sign per channel"""
    B, heads, Tq, Tk = shape
    kpi, ones = ar.kernel_model(d)
    p = ar.uniform("straddle", B, heads, Tq, Tk, d, cancelling=True)
    assert ar.check_exact(p, ar.emulate(p.q, p.k, p.v, heads, False, kpi, ones)) is None
    got = ar.emulate(p.q, p.k, p.v, heads, False, kpi, ones, adder="truncating")
    assert ar.check_exact(p, got) is not None
    zero = p.expect == 0
    assert zero.any() and (got[zero] <= 0).all() and (got[zero] < 0).any() and (got[zero] >= -2.0 ** -21).all()


def _acts(defect, heads, Tq, Tk, causal, kpi):
    if defect == "drop_last_key":
        return Tk % kpi != 0
    if defect == "include_past_key":
        return Tk % kpi != 0 and not causal          # causal: key Tk lies behind every query
    if defect == "swap_v_slots":
        return Tk >= 2
    if defect == "skip_rescale":
        return Tk > kpi
    if defect == "causal_ge":
        return causal
    if defect == "next_head_v":
        return heads >= 2
    raise ValueError(defect)


@pytest.mark.parametrize("defect", ar.DEFECTS)
def test_every_seeded_defect_is_caught_where_it_can_act(defect):
    acted = 0
    for (B, heads, Tq, Tk), causal in ALL_SHAPES:
        for d in (8, 40):
            ones = ar.kernel_model(d)[1]
            exact = traj = None
            for kpi in (32, 64):
                if not _acts(defect, heads, Tq, Tk, causal, kpi):
                    continue
                if exact is None:
                    exact = ar.exact_probes(B, heads, Tq, Tk, d, causal)
                    traj = ar.trajectory_probes(B, heads, Tq, Tk, d, causal)
                    traj = list(zip(traj, ar.references(traj)))
                acted += 1
                failed = {p.name.split("/")[0] for p in exact if ar.check_exact(p, _run(p, kpi, ones, defect)) is not None}
                failed |= {p.name.split("/")[0] for p, (ref, spread) in traj
                           if not ar.err_over_tol(_run(p, kpi, ones, defect), ref, spread, p.v, Tk) < 1.0}
                assert failed, f"{defect} survives at {(B, heads, Tq, Tk)} causal={causal} d={d} keys_per_iter={kpi}"
    assert acted >= 4
