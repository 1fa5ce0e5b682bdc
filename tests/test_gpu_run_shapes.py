"""GPU: the kernels behind NeRFRenderer.run (csrc/render.hip: k_sample_coarse, k_sample_fine_merge, k_sample_pdf, k_composite_run_fwd / bwd,
k_recon_loss) away from the golden scene — against the float64 restatement (tests/run_restatement.py) at the ragged sample counts, the ray
counts around the four-rays-per-workgroup edge and the rays near_far_from_aabb really produces: from outside, from inside, missing the box,
looking away from it (far < near: descending samples), starting on a slab plane with a zero direction component (NaN near) and
axis-parallel.  Inputs come from tests/run_testlib.py; tests/test_run_restatement_host.py checks on the CPU what is assumed about them.

The merge invariants come first: they are what makes the indexed compositing kernels memory-safe, and nothing in that test hands an
index to another kernel.  The end-to-end test at the bottom checks the same invariant before its first compositing call."""
import functools
import math

import numpy as np
import pytest
import torch

import run_restatement as rr
import run_testlib as tl

pytestmark = pytest.mark.gpu

from oracle.toy_field import ToyField      # noqa: E402

SENT_F = 0x7FC0BEEF                        # a NaN no arithmetic produces
SENT_I = -1                                # 0xFFFFFFFF


def _sent_f(*shape):
    return torch.full(shape, SENT_F, dtype=torch.int32, device="cuda").view(torch.float32)


def _sent_i(*shape):
    return torch.full(shape, SENT_I, dtype=torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _written(*tensors):
    return all(bool((_bits(t) != (SENT_F if t.is_floating_point() else SENT_I)).all()) for t in tensors)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _cpu(d):
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _merge_run(case):
    """one configuration through cnerf_sample_coarse and the three forms of the merge, every output pre-filled with a sentinel (the
    wrappers' torch.empty can hand back a buffer that holds an earlier, valid result) -> CPU tensors"""
    from customnerf_amd import raymarching
    from customnerf_amd._lib import lib, check, ptr, stream
    from customnerf_amd.nerf import render_ops
    T, t, N, det, bound = case[:5]
    S = T + t
    o, d, cls, noise, sigma, u = tl.merge_inputs(case)
    o, d, noise, sigma, aabb = o.cuda(), d.cuda(), noise.cuda(), sigma.cuda(), tl.aabb_of(bound).cuda()
    u = None if u is None else u.cuda()
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, tl.MIN_NEAR)
    zc, xc = render_ops.sample_coarse(o, d, nears, fars, aabb, T, noise)
    args = (ptr(o), ptr(d), ptr(nears), ptr(fars), ptr(aabb), ptr(zc), ptr(sigma), ptr(u), N, T, t)
    za, xf, src = _sent_f(N, S), _sent_f(N, t, 3), _sent_i(N, S)
    check(lib.cnerf_sample_fine_merge_split(*args, ptr(za), None, ptr(xf), ptr(src), stream()), "split")
    za_u, xf_u, src_u, unit = _sent_f(N, S), _sent_f(N, t, 3), _sent_i(N, S), _sent_f(N, t, 3)
    check(lib.cnerf_sample_fine_merge_split_unit(*args, ptr(za_u), ptr(xf_u), ptr(src_u), ptr(unit), float(bound), stream()), "split_unit")
    za_m, xa_m = _sent_f(N, S), _sent_f(N, S, 3)
    check(lib.cnerf_sample_fine_merge(*args, ptr(za_m), ptr(xa_m), stream()), "merged")
    written = _written(za, xf, src, za_u, xf_u, src_u, unit, za_m, xa_m)
    unit_ok = torch.equal(unit, (xf_u + bound) / (2 * bound))          # on the device, where torch divides as the kernel does (grid.py:156)
    return _cpu(dict(cls=cls, nears=nears, fars=fars, zc=zc, xc=xc, sigma=sigma, u=u, za=za, xf=xf, src=src, za_u=za_u, xf_u=xf_u, src_u=src_u,
                     unit=unit, za_m=za_m, xa_m=xa_m, written=written, unit_ok=unit_ok))


def _cases(T, t):
    return [c for c in tl.merge_cases() if c[:2] == (T, t)]


@pytest.mark.parametrize("T,t", tl.MERGE_TT)
def test_merge_writes_a_permutation_in_sort_order_for_every_ray(T, t):
    """k_sample_fine_merge, split, split + grid coordinates and merged form, N in {1, 3, 4, 5, 64}, random (with repeated values) and det u,
    bounds 2 and 1.3, all ray and sigma classes: every output element is written; every row of src_index is a permutation of its ray's
    rows (n*T .. n*T+T-1 and N*T+n*t .. N*T+n*t+t-1); z_all holds the coarse samples' bits where src_index says they are and is in
    torch.sort's order (ascending, NaN last); the three forms agree bit for bit; the merged form's positions are those of the sample list
    gathered through src_index.  The rank rules of the fast path hold for ascending, comparable samples only: a ray looking away from
    the box (descending samples) or with a NaN near left up to half of its positions unwritten before the general path existed."""
    for case in _cases(T, t):
        r = _merge_run(case)
        N, bound = case[2], case[4]
        S = T + t
        if N == 64:
            tl.assert_ray_classes(r["cls"], r["nears"], r["fars"])
        assert r["written"], (case, "an output element was left unwritten")
        assert tl.is_row_permutation(r["src"], N, T, t), case
        src = r["src"].long()
        coarse = src < N * T
        assert torch.equal(_bits(r["za"])[coarse], _bits(r["zc"]).reshape(-1)[src[coarse]]), case
        assert tl.in_sort_order(r["za"]), case
        assert _same_bits(r["za"], r["za_m"]) and _same_bits(r["za"], r["za_u"]) and torch.equal(r["src"], r["src_u"]), case
        assert _same_bits(r["xf"], r["xf_u"]), case
        rows = torch.cat([r["xc"].reshape(-1, 3), r["xf"].reshape(-1, 3)])
        assert _same_bits(rows[src], r["xa_m"]), case
        assert r["unit_ok"], case


def _fine_samples(r, N, T, t):
    """the new samples in draw order, read out of z_all through src_index"""
    src = r["src"].long()
    fine = src >= N * T
    m = src - N * T - torch.arange(N)[:, None] * t
    nz = torch.full((N, t), float("nan"))
    nz[torch.nonzero(fine)[:, 0], m[fine]] = r["za"][fine]
    return nz


@pytest.mark.parametrize("T,t", tl.MERGE_TT)
def test_fine_samples_against_float64(T, t):
    """the inverse-CDF samples of k_sample_fine_merge against the float64 chain (weights -> pdf -> cdf -> searchsorted -> interpolation) on
    the kernel's own coarse samples, over the configurations of the merge test, for the rays with a proper pdf (finite, ascending coarse
    samples).  A draw within EPS = 2^-20 (16 float32 ulp of 1) of the `denom < 1e-5` rule, or of a CDF step next to a bin under that
    rule, is ill-conditioned: it need only lie inside the ray's bins, and at most 2 % of a configuration's draws may be such.  Every other
    draw: |z - z64| <= |bins_a - bins_b| 2 EPS / denom64 + 8 ulp32(max |bins|), or the bound of run_restatement.near_step next to a step.
    Measured on MI355X, worst configuration per (T, t) — share of ill-conditioned draws / worst error over bound:
    (3,2) 0 / 0.06, (4,3) 0 / 0.07, (16,48) 0.06 % / 0.79, (63,5) 0 / 0.11, (64,64) 0.04 % / 0.14, (65,63) 0 / 0.18, (100,7) 0.41 % / 0.16,
    (128,127) 0.26 % / 0.28, (128,128) 0.11 % / 0.39."""
    worst_share, worst_ratio = 0.0, 0.0
    for case in _cases(T, t):
        r = _merge_run(case)
        N, det = case[2], case[3]
        assert tl.is_row_permutation(r["src"], N, T, t), case
        nz = _fine_samples(r, N, T, t)
        w, mid = rr.coarse_weights(r["zc"], r["sigma"], r["nears"], r["fars"], T)
        with np.errstate(all="ignore"):
            d = rr.sample_pdf_detail(mid, w[:, 1:-1], t, det=det, u=r["u"])
        ok = rr.usable_rows(d, w) & torch.isfinite(r["zc"]).all(-1)
        if not bool(ok.any()):
            continue
        share, ratio = rr.check_fine(nz[ok], {k: v[ok] for k, v in d.items()})
        worst_share, worst_ratio = max(worst_share, share), max(worst_ratio, ratio)
        assert share <= 0.02, (case, share)
        assert ratio <= 1.0, (case, ratio)
    print(f"fine samples T={T} t={t}: worst ill-conditioned share {worst_share:.4f}, worst error / bound {worst_ratio:.3f}")


@pytest.mark.parametrize("n_bins", tl.PDF_BINS)
def test_sample_pdf_kernel_against_float64(n_bins):
    """cnerf_sample_pdf on its own: n_samples in {1, 2, 63, 64, 65, 200}, B in {1, 5}, det and random u, all-zero weights and a spike; the
    rule and the cap of test_fine_samples_against_float64.  Measured on MI355X: no ill-conditioned draw in any configuration (the det
    draws that meet a uniform CDF on its steps fall under near_step's bound); worst error over bound 0.05 to 0.09 per n_bins."""
    from customnerf_amd.nerf.renderer import sample_pdf
    worst_share, worst_ratio = 0.0, 0.0
    for ns in tl.PDF_SAMPLES:
        for B in tl.PDF_B:
            for kind in ("zero", "spike"):
                bins, w = tl.pdf_inputs(n_bins, B, kind)
                for det in (True, False):
                    u = None if det else tl.pdf_u(B, ns)
                    out = sample_pdf(bins.cuda(), w.cuda(), ns, det=det, u=None if det else u.cuda()).cpu()
                    assert out.shape == (B, ns)
                    share, ratio = rr.check_fine(out, rr.sample_pdf_detail(bins, w, ns, det=det, u=u))
                    worst_share, worst_ratio = max(worst_share, share), max(worst_ratio, ratio)
                    assert share <= 0.02 and ratio <= 1.0, (n_bins, ns, B, kind, det, share, ratio)
    print(f"sample_pdf n_bins={n_bins}: worst ill-conditioned share {worst_share:.4f}, worst error / bound {worst_ratio:.3f}")


@pytest.mark.parametrize("T", tl.COARSE_T)
def test_coarse_sampler_against_float64(T):
    """cnerf_sample_coarse / _unit / _unit_aabb, N in {1, 5, 1000}, with and without jitter, bounds 2 and 1.3, all ray classes: z within 4
    float32 ulp of max(|near|, |far|) of float64 (subtract, linspace, multiply, add, the jitter term), exactly FLT_MAX on a ray that misses
    and NaN on a NaN ray; xyz within 2e-6 max(1, |x|); the form with the slab test folded in equals the two launches bit for bit"""
    from customnerf_amd import raymarching
    from customnerf_amd.nerf import render_ops
    for k, N in enumerate(tl.COARSE_N):
        for bound in tl.BOUNDS:
            o, d, cls = tl.make_rays(bound, -(-max(N, 12) // 6), seed=int(bound * 10))
            first = 0 if N == 1000 else (tl.COARSE_T.index(T) + 3 * k) % 6
            o, d, cls = o[first:first + N].contiguous(), d[first:first + N].contiguous(), cls[first:first + N]
            aabb = tl.aabb_of(bound)
            nears, fars = raymarching.near_far_from_aabb(o.cuda(), d.cuda(), aabb.cuda(), tl.MIN_NEAR)
            if N == 1000:
                tl.assert_ray_classes(cls, nears, fars)
            kind = tl.classify(nears, fars)
            for jitter in (False, True):
                noise = torch.rand(N, T, generator=torch.Generator().manual_seed(T + N)) if jitter else None
                nz = None if noise is None else noise.cuda()
                unit_a, xyz_b, unit_b = _sent_f(N, T, 3), _sent_f(N, T, 3), _sent_f(N, T, 3)
                z, xyz = render_ops.sample_coarse(o.cuda(), d.cuda(), nears, fars, aabb.cuda(), T, nz)
                z_a, xyz_a = render_ops.sample_coarse(o.cuda(), d.cuda(), nears, fars, aabb.cuda(), T, nz, unit_out=unit_a, bound=bound)
                n_b, f_b, z_b, _ = render_ops.sample_coarse_aabb(o.cuda(), d.cuda(), aabb.cuda(), tl.MIN_NEAR, T, nz, xyz_b, unit_b, bound)
                assert _written(unit_a, xyz_b, unit_b)
                assert _same_bits(n_b, nears) and _same_bits(f_b, fars)
                assert _same_bits(z, z_a) and _same_bits(z, z_b) and _same_bits(xyz, xyz_a) and _same_bits(xyz, xyz_b) and _same_bits(unit_a, unit_b)
                z64, xyz64 = rr.sample_coarse(o, d, nears.cpu(), fars.cpu(), aabb, T, noise)
                z, xyz = z.cpu().double(), xyz.cpu().double()
                miss, nan = torch.from_numpy(kind == "miss"), torch.from_numpy(kind == "nan")
                assert bool((z[miss] == tl.FLT_MAX).all()) and bool(torch.isnan(z[nan]).all())
                rest = ~miss & ~nan
                tol = 4 * rr.ulp32(torch.maximum(nears.cpu().abs(), fars.cpu().abs()))[:, None]
                assert bool(((z - z64).abs() <= tol)[rest].all()), (T, N, bound, jitter, float(((z - z64).abs() / tol)[rest].max()))
                assert bool(((xyz - xyz64).abs() <= 2e-6 * xyz64.abs().clamp(min=1.0))[~nan].all()), (T, N, bound, jitter)


COMPOSITE_CFG = [  # soft mask, conf_thr, detach_bg, detach_mask
    (True, 0.5, False, False), (True, 0.3, True, True), (False, 0.5, True, False), (False, 0.5, False, True)]


def _composite_kernels(sig, rgbc, z, nears, fars, src, num_steps, soft, thr, dbg, dmask, variants, g):
    """forward + backward through the library binding on sentinel-filled outputs; sig / rgbc in sample-list order (src None: plain)"""
    from customnerf_amd._lib import lib, check, ptr, stream
    N, S = z.shape
    out, gs, gc = _sent_f(3, N, 6), _sent_f(N * S), _sent_f(N * S, 4)
    check(lib.cnerf_composite_run_indexed_variants(ptr(sig), ptr(rgbc), ptr(z), ptr(nears), ptr(fars), N, S, num_steps, int(soft), float(thr), ptr(src),
                                                   ptr(out), None, None, None, variants, stream()), "composite")
    check(lib.cnerf_composite_run_backward_indexed(ptr(g), ptr(sig), ptr(rgbc), ptr(z), ptr(nears), ptr(fars), N, S, num_steps, int(soft), float(thr),
                                                   int(dbg), int(dmask), ptr(src), ptr(gs), ptr(gc), stream()), "composite backward")
    assert _written(out, gs, gc)
    return out.cpu().double(), gs.cpu().double(), gc.cpu().double()


def _check_backward(name, got, ref64, ref32, where):
    """the kernel's gradient within 4 x the float32 oracle's own distance from float64 (two legal float32 summation orders: wave scan here,
    sequential cumprod there) + 1e-5 max(1, max |ref|); NaN exactly where float64 is NaN.  -> (kernel error / oracle error, kernel error /
    tolerance).  The first ratio is large where the oracle happens to be exact (a zero-sigma ray: 1e-15 against the kernel's 1e-8)."""
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), (where, name, "NaN pattern")
    fin = torch.isfinite(ref64)
    if not bool(fin.any()):
        return 0.0, 0.0
    err_k = float((got - ref64)[fin].abs().max())
    e32 = (ref32.double() - ref64)[fin & torch.isfinite(ref32.double())].abs()
    err_o = float(e32.max()) if e32.numel() else 0.0
    tol = 4 * err_o + 1e-5 * max(1.0, float(ref64[fin].abs().max()))
    assert err_k <= tol, (where, name, err_k, err_o, tol)
    return (err_k / err_o if err_o > 0 else 0.0), err_k / tol


def _check_composite(where, out, gs, gc, ref64, ref32, variants):
    o64, gs64, gc64 = ref64
    rows = [0] if variants == 1 else [0, 1, 2]
    if variants == 1:
        assert float(out[1:].abs().max()) == 0.0, where
    assert torch.equal(torch.isnan(out[rows]), torch.isnan(o64[rows])), (where, "NaN pattern of the forward")
    fin = ~torch.isnan(o64[rows])
    err = float((out[rows] - o64[rows])[fin].abs().max())
    assert err <= 2e-6, (where, "forward", err)
    return (err,) + _check_backward("g_sigma", gs, gs64, ref32[1], where) + _check_backward("g_rgbc", gc, gc64, ref32[2], where)


@pytest.mark.parametrize("S", tl.COMPOSITE_S)
def test_composites_forward_and_backward_against_float64_autograd(S):
    """k_composite_run_fwd / bwd, N in {1, 5}, plain and through a random per-ray permutation, variants 7 and 1, soft mask with conf_thr 0.5
    and 0.3, hard mask with confidences of exactly 0.5, both detach flags; rows: random, zero sigma, an opaque first sample (q = 1e-15 under
    the suffix division), descending z, a ray that misses the box (depth and what depends on it NaN exactly where float64 has NaN).
    Forward: 2e-6 absolute.  Backward: 4 x the float32 oracle's own error against float64 + 1e-5 max(1, max |ref|).
    Measured on MI355X, worst over the 64 combinations of each S: forward error 5.5e-8 (S = 1) to 1.5e-6 (S = 256).  Backward, kernel
    error over the float32 oracle's error: g_rgbc 1.0 to 11.2 (S = 255), g_sigma 1.0 to 3.5 where the oracle errs at all and up to 3e7 on
    the rows where it is exact to 1e-15 (zero sigma) and the kernel to 1e-8; kernel error over the tolerance: g_sigma at most 0.042,
    g_rgbc at most 0.325 (S = 64) — wherever the first ratio exceeds 4 it is the 1e-5 max(1, max |ref|) term that admits the kernel."""
    worst = [0.0] * 5
    for ci, (soft, thr, dbg, dmask) in enumerate(COMPOSITE_CFG):
        for N in (1, 5):
            first = (tl.COMPOSITE_S.index(S) + ci) % 5
            sig, rgbc, z, nears, fars = tl.composite_inputs(N, S, first=first, seed=ci, exact_half_conf=not soft)
            num_steps = max(1, S // 2)
            gen = torch.Generator().manual_seed(100 * S + ci)
            perm = torch.stack([torch.randperm(S, generator=gen) for _ in range(N)]) + torch.arange(N)[:, None] * S
            for variants in (7, 1):
                g = torch.randn(3, N, 6, generator=gen)
                if variants == 1:
                    g[1:] = 0
                ref64 = rr.composites_with_grads(sig, rgbc, z, nears, fars, num_steps, soft, thr, g, dbg, dmask)
                ref32 = rr.composites_with_grads(sig, rgbc, z, nears, fars, num_steps, soft, thr, g, dbg, dmask, dtype=torch.float32)
                for indexed in (False, True):
                    where = (S, N, soft, thr, dbg, dmask, variants, indexed, tl.COMPOSITE_ROWS[first])
                    if indexed:
                        s_list, c_list = torch.empty(N * S), torch.empty(N * S, 4)
                        s_list[perm.reshape(-1)], c_list[perm.reshape(-1)] = sig.reshape(-1), rgbc.reshape(-1, 4)
                        src = perm.int().cuda()
                    else:
                        s_list, c_list, src = sig.reshape(-1), rgbc.reshape(-1, 4), None
                    out, gs, gc = _composite_kernels(s_list.cuda(), c_list.contiguous().cuda(), z.cuda(), nears.cuda(), fars.cuda(), src, num_steps, soft,
                                                     thr, dbg, dmask, variants, g.cuda())
                    if indexed:
                        gs, gc = gs[perm.reshape(-1)], gc[perm.reshape(-1)]
                    res = _check_composite(where, out, gs.view(N, S), gc.view(N, S, 4), ref64, ref32, variants)
                    worst = [max(a, b) for a, b in zip(worst, res)]
    print(f"composites S={S}: forward max error {worst[0]:.2e}; backward, worst kernel error / float32 oracle error and / tolerance: "
          f"g_sigma {worst[1]:.3g} and {worst[2]:.3f}, g_rgbc {worst[3]:.3g} and {worst[4]:.3f}")


@pytest.mark.parametrize("T,t", tl.FLUSH_TT)
def test_early_termination_flags_of_the_compositing_backward(T, t):
    """cnerf_composite_run_backward_indexed_flush with and without flush_half_zero, half the rays turning opaque along the way: every row of the
    flushed gradients is the unflushed row bit for bit or exactly zero; a zeroed row's unflushed gradients round to zero in half as the field
    backward forms them, half(g_sigma clamp(sigma, e^-15, e^15)) and half(g_c c (1 - c)); tile_live[k] == 1 exactly when the 32-row tile k
    of the sample list holds a row with a nonzero or non-finite flushed gradient"""
    from customnerf_amd._lib import lib, check, ptr, stream
    N, S = 8, T + t
    gen = torch.Generator().manual_seed(T * 1000 + t)
    zc = torch.sort(torch.rand(N, T, generator=gen) * 3 + 0.3, dim=-1).values
    zf = torch.rand(N, t, generator=gen) * 3 + 0.3
    z, order = torch.sort(torch.cat([zc, zf], 1), dim=1)
    n = torch.arange(N)[:, None]
    src = torch.where(order < T, n * T + order, N * T + n * t + (order - T))
    assert tl.is_row_permutation(src, N, T, t)
    sig = torch.rand(N, S, generator=gen) * 2
    sig[1::2, S // 4:] = 40.0                                              # transmittance fades over some twenty samples, then underflows
    rgbc = torch.rand(N, S, 4, generator=gen) * 0.9 + 0.05
    s_list, c_list = torch.empty(N * S), torch.empty(N * S, 4)
    s_list[src.reshape(-1)], c_list[src.reshape(-1)] = sig.reshape(-1), rgbc.reshape(-1, 4)
    nears, fars = (z[:, 0] - 0.05).contiguous(), (z[:, -1] + 0.2).contiguous()
    g = torch.randn(3, N, 6, generator=gen)
    dev = [a.cuda() for a in (g, s_list, c_list, z, nears, fars, src.int())]
    res = []
    for flush in (0, 1):
        gs, gc = _sent_f(N * S), _sent_f(N * S, 4)
        live = torch.full((N * S // 32,), 0x5A, dtype=torch.uint8, device="cuda") if flush else None
        check(lib.cnerf_composite_run_backward_indexed_flush(*[ptr(a) for a in dev[:6]], N, S, T, 1, 0.5, 0, 0, ptr(dev[6]), ptr(gs), ptr(gc), flush,
                                                             ptr(live), stream()), "flush")
        assert _written(gs, gc)
        res.append((gs.cpu(), gc.cpu(), None if live is None else live.cpu()))
    (gs0, gc0, _), (gs1, gc1, live) = res
    row0, row1 = torch.cat([gs0[:, None], gc0], 1), torch.cat([gs1[:, None], gc1], 1)
    same = (_bits(row0) == _bits(row1)).all(1)
    zero = (row1 == 0).all(1) & (_bits(row1) == 0).all(1)
    assert bool((same | zero).all())
    flushed = zero & ~same
    sc = torch.clamp(s_list, math.exp(-15.0), math.exp(15.0))
    assert bool(((gs0 * sc).half()[flushed] == 0).all()) and bool(((gc0 * (c_list * (1 - c_list))).half()[flushed] == 0).all())
    want = ((row1 != 0) | ~torch.isfinite(row1)).any(1).view(-1, 32).any(1)
    assert set(live.tolist()) <= {0, 1} and torch.equal(live.bool(), want)
    assert int(flushed.sum()) > 0 and bool(want.any())                 # rows were flushed, tiles lived
    assert T < 64 or not bool(want.all())                              # and with more than one coarse tile per ray, the far ones died


@pytest.mark.parametrize("with_mask", [True, False])
def test_recon_loss_at_the_block_edges_back_to_back(with_mask):
    """cnerf_recon_loss and cnerf_recon_loss_scaled, N in {1, 255, 256, 257, 16384, 16385, 40000} (one thread, one workgroup and one more,
    all 64 workgroups and one more ray, the grid-stride loop), launched back to back on one stream — the second launch finds the ticket
    the first one's last workgroup must have reset — against float64, with the tolerances of
    test_fused_recon_loss_matches_the_torch_formulation"""
    from customnerf_amd._lib import lib, check, ptr, stream
    gen = torch.Generator().manual_seed(7)
    scale = torch.tensor([4096.0], device="cuda")
    for N in tl.RECON_N:
        outs = [torch.rand(3, N, 6, generator=gen) for _ in range(2)]
        rgb, mask = torch.rand(N, 3, generator=gen), ((torch.rand(N, generator=gen) > 0.5).float() if with_mask else None)
        w_conf = 0.3 if with_mask else 0.0
        dev = [a.cuda() for a in outs] + [rgb.cuda(), None if mask is None else mask.cuda()]
        la, ga, lb, gb = _sent_f(65), _sent_f(3, N, 6), _sent_f(65), _sent_f(3, N, 6)
        check(lib.cnerf_recon_loss(ptr(dev[0]), ptr(dev[2]), ptr(dev[3]), N, 1.0, w_conf, ptr(la), ptr(ga), stream()), "recon_loss")
        check(lib.cnerf_recon_loss_scaled(ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), N, 1.0, w_conf, ptr(scale), ptr(lb), ptr(gb), stream()), "recon_loss_scaled")
        assert _written(ga, gb, la[:1], lb[:1])
        for out, loss, grad, k in ((outs[0], la, ga, 1.0), (outs[1], lb, gb, 4096.0)):
            l64, g64 = rr.recon_loss(out, rgb, mask, 1.0, w_conf)
            assert abs(float(loss[0]) - float(l64)) < 1e-6 * max(1.0, float(l64)), (N, k, float(loss[0]), float(l64))
            assert torch.allclose(grad.cpu().double(), g64 * k, atol=1e-9 * k, rtol=1e-5), (N, k)
            assert bool((grad[1:] == 0).all())


@pytest.mark.parametrize("T,t,bound", [(32, 32, 2.0), (16, 48, 1.3)])
def test_run_steps_end_to_end_on_every_ray_class(T, t, bound):
    """What run() does, by hand on one batch that holds every ray class: sample_coarse_aabb, the toy field, sample_fine_merge_split,
    composite_run_indexed and its backward.  src_index is checked to be a permutation of every ray's rows BEFORE it reaches a compositing
    kernel.  Against float64 on the kernel's sorted samples, ray by ray: rays with finite samples within the tolerances of the composite
    test; a NaN ray has NaN exactly where float64 has; the gradients of the ordinary rays are finite.  Measured on MI355X: forward error
    4.6e-7 / 3.5e-7, kernel error over tolerance at most 0.32."""
    from customnerf_amd.nerf import render_ops
    N = 66
    S = T + t
    o, d, cls = tl.make_rays(bound, 11, seed=int(bound * 10))
    gen = torch.Generator().manual_seed(T + t)
    noise, u, g = torch.rand(N, T, generator=gen), tl.make_u(N, t, seed=T), torch.randn(3, N, 6, generator=gen)
    aabb = tl.aabb_of(bound).cuda()
    field = ToyField()
    xc, unit = _sent_f(N, T, 3), _sent_f(N, T, 3)
    nears, fars, zc, _ = render_ops.sample_coarse_aabb(o.cuda(), d.cuda(), aabb, tl.MIN_NEAR, T, noise.cuda(), xc, unit, bound)
    tl.assert_ray_classes(cls, nears, fars)
    sig_c = field.density(xc.reshape(-1, 3))['sigma'].view(N, T).contiguous()
    za, xf, src = render_ops.sample_fine_merge_split(o.cuda(), d.cuda(), nears, fars, aabb, zc, sig_c, t, u.cuda())
    assert tl.is_row_permutation(src, N, T, t)                         # no unchecked index reaches a kernel
    assert tl.in_sort_order(za)
    rows = torch.cat([xc.reshape(-1, 3), xf.reshape(-1, 3)])
    dirs = torch.cat([d.cuda().repeat_interleave(T, 0), d.cuda().repeat_interleave(t, 0)])
    s_list, c_list, _ = field(rows, dirs)
    s_list, c_list = s_list.detach().contiguous().requires_grad_(True), c_list.detach().contiguous().requires_grad_(True)
    out = render_ops.composite_run_indexed(s_list, c_list, za, src, nears, fars, T, True, 0.5)
    (out * g.cuda()).sum().backward()
    idx = src.long().cpu()
    sig, rgbc = s_list.detach().cpu()[idx], c_list.detach().cpu()[idx]
    gs, gc = s_list.grad.cpu().double()[idx], c_list.grad.cpu().double()[idx]
    out = out.detach().cpu().double()
    ref64 = rr.composites_with_grads(sig, rgbc, za, nears, fars, T, True, 0.5, g)
    ref32 = rr.composites_with_grads(sig, rgbc, za, nears, fars, T, True, 0.5, g, dtype=torch.float32)
    kind = tl.classify(nears, fars)
    finite_z = torch.isfinite(za.cpu()).all(-1)
    nan = torch.from_numpy(kind == "nan")
    assert bool(nan.any()) and not bool(finite_z[nan].any())
    for name, got, want in (("out", out.permute(1, 0, 2), ref64[0].permute(1, 0, 2)), ("g_sigma", gs, ref64[1]), ("g_rgbc", gc, ref64[2])):
        assert torch.equal(torch.isnan(got[nan]), torch.isnan(want[nan])), (name, "NaN pattern of the NaN rays")
    rest = finite_z & ~nan                                             # (a ray looking away whose coarse weights overflowed has NaN samples of its own)
    sel = lambda a, dim: a.index_select(dim, torch.nonzero(rest)[:, 0])
    res = _check_composite((T, t, bound), sel(out, 1), sel(gs, 0), sel(gc, 0), [sel(ref64[0], 1), sel(ref64[1], 0), sel(ref64[2], 0)],
                           [sel(ref32[0], 1), sel(ref32[1], 0), sel(ref32[2], 0)], 7)
    valid = torch.from_numpy(kind == "valid") & finite_z
    assert bool(valid.any()) and bool(torch.isfinite(gs[valid]).all()) and bool(torch.isfinite(gc[valid]).all())
    print(f"run steps T={T} t={t} bound={bound}: forward max error {res[0]:.2e}; backward, kernel error / float32 oracle error and / tolerance: "
          f"g_sigma {res[1]:.3g} and {res[2]:.3f}, g_rgbc {res[3]:.3g} and {res[4]:.3f}")
