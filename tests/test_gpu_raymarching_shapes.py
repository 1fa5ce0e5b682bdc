"""GPU parity of the ray march and the compositing kernels (csrc/raymarching.hip) away from the one scene of tests/test_gpu_raymarching.py
(bound 2, two cascades, 128^3, pinhole rays from outside the box, ray counts that are multiples of 64): one to five cascades, a bound that
is no power of two, rays with +0 / -0 direction components and rays that start inside the box, a prime ray count and ray counts below one
workgroup, a compositing table whose events sit on the 64-sample chunk boundary of the wave kernels and whose output slots are permuted.
The judge is the C oracle (oracle/raymarching_ref.c), pinned to its numpy twin on the same cases in tests/test_oracle_independent.py;
integer outputs and everything the march writes are compared bit for bit.  Inputs and what they must contain: tests/march_testlib.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_oracle as co          # noqa: E402  (checker only)

import march_testlib as ML                 # noqa: E402

BIG_ROWS = ((4.0, 64), (16.0, 32))         # the rows with three and five cascades: both writers and the fixed budget are run on these


@pytest.fixture(scope="module")
def rm():
    from customnerf_amd import raymarching
    return raymarching


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                           # a copy: the shared cases are read-only


def gpu_march(rm, bound, H, dt_gamma, max_steps, N=ML.N_RAYS, mean_count=-1, force_all_rays=True, noises=None):
    c = ML.march_case(bound, H)
    counter = torch.zeros(2, dtype=torch.int32).cuda()
    noises = c["noises"][:N] if noises is None else noises
    x, d, l, r = rm.march_rays_train(cuda(c["o"][:N]), cuda(c["d"][:N]), bound, cuda(c["bitfield"]), c["C"], H, cuda(c["nears"][:N]),
                                     cuda(c["fars"][:N]), counter, mean_count, True, 128, force_all_rays, dt_gamma, max_steps, noises=cuda(noises))
    return x.cpu().numpy(), d.cpu().numpy(), l.cpu().numpy(), r.cpu().numpy(), counter.cpu().numpy().tolist()


def assert_same_march(got, want, N):
    x, d, l, r, counter = got
    xr, dr, lr, rr = want
    np.testing.assert_array_equal(r, rr)                                  # (ray id, offset, num_steps): ray-ordered
    assert counter == [int(rr[:, 2].sum()), N]
    assert x.shape == xr.shape and d.shape == dr.shape and l.shape == lr.shape
    np.testing.assert_array_equal(x, xr)
    np.testing.assert_array_equal(d, dr)
    np.testing.assert_array_equal(l, lr)


@pytest.mark.parametrize("dt_gamma,max_steps", ML.SETTINGS)
@pytest.mark.parametrize("bound,H", ML.CONFIGS)
def test_march_matrix_bit_exact(rm, bound, H, dt_gamma, max_steps):
    c = ML.march_case(bound, H)
    n, f = rm.near_far_from_aabb(cuda(c["o"]), cuda(c["d"]), cuda(c["aabb"]), 0.05)
    np.testing.assert_array_equal(n.cpu().numpy(), c["nears"])
    np.testing.assert_array_equal(f.cpu().numpy(), c["fars"])
    want = ML.march_oracle(bound, H, dt_gamma, max_steps)
    steps = want[3][:, 2]
    assert (steps == 0).any()                                             # rays without a step
    assert set(ML.sample_levels(want[0][:int(steps.sum())], c["C"]).tolist()) == set(range(c["C"]))     # every cascade level is sampled
    if ((bound, H), (dt_gamma, max_steps)) in ML.CAPPED:
        assert int(steps.max()) == max_steps                              # the step cap is reached
    assert_same_march(gpu_march(rm, bound, H, dt_gamma, max_steps), want, ML.N_RAYS)


@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 32])
@pytest.mark.parametrize("bound,H", ML.CONFIGS[:2])
def test_march_dt_min_above_dt_max(rm, bound, H, dt_gamma):
    """max_steps = 16 on the two fine grids: dt_min = 2 sqrt3 / 16 is twice dt_max = 2 sqrt3 2^(C-1) / H, and clamp(x, dt_min, dt_max) is
    dt_max whatever x is — also with a dt_gamma that would otherwise grow the step along the ray"""
    max_steps = 16
    assert 1.0 / max_steps > 2 ** (ML.cascades(bound) - 1) / H
    want = ML.march_oracle(bound, H, dt_gamma, max_steps)
    total = int(want[3][:, 2].sum())
    assert total > 5 * ML.N_RAYS and np.all(want[2][:total, 0] == np.float32(2 * np.sqrt(3) * 2 ** (ML.cascades(bound) - 1) / H))     # one step: dt_max
    assert_same_march(gpu_march(rm, bound, H, dt_gamma, max_steps), want, ML.N_RAYS)


@pytest.mark.parametrize("dt_gamma,max_steps", ML.SETTINGS)
@pytest.mark.parametrize("bound,H", BIG_ROWS)
def test_march_both_writers_agree(rm, monkeypatch, bound, H, dt_gamma, max_steps):
    """the writer that replays the probe list of the counting pass and the one that marches again (taken above _HITS_MAX_BYTES)"""
    from customnerf_amd.raymarching import raymarching as rmod
    from_hits = gpu_march(rm, bound, H, dt_gamma, max_steps)
    monkeypatch.setattr(rmod, "_HITS_MAX_BYTES", 1 << 16)
    assert ML.N_RAYS * max_steps * 8 > rmod._HITS_MAX_BYTES
    remarched = gpu_march(rm, bound, H, dt_gamma, max_steps)
    assert rmod.scratch_key(torch.device("cuda", torch.cuda.current_device())) not in rmod._HITS
    assert_same_march(remarched, ML.march_oracle(bound, H, dt_gamma, max_steps), ML.N_RAYS)
    for a, b in zip(from_hits[:4], remarched[:4]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dt_gamma,max_steps", ML.SETTINGS)
@pytest.mark.parametrize("bound,H", BIG_ROWS)
def test_march_fixed_budget(rm, bound, H, dt_gamma, max_steps):
    """a budget of 60 % of what the rays need: the scan starts at ray floor(noises[0] * N) and wraps, a kept prefix is followed by the
    dropped run, and the kept rays hold the exact-size march's samples bit for bit (the assertions of
    test_march_rays_train_budget_overflow_is_not_tied_to_image_position)"""
    c = ML.march_case(bound, H)
    N = ML.N_RAYS
    for frac in (0.0, 0.37, 0.93):
        nz = c["noises"].copy()
        nz[0] = frac                                                        # also ray 0's own jitter: re-march the reference samples with it
        xr, dr, lr, rr = co.march_rays_train(c["o"], c["d"], bound, c["bitfield"], c["C"], H, c["nears"], c["fars"], None, -1, nz, 128, True,
                                             dt_gamma, max_steps)
        total = int(rr[:, 2].sum())
        M = (total * 6 // 10) // 128 * 128
        x, dd, l, r, counter = gpu_march(rm, bound, H, dt_gamma, max_steps, mean_count=M - 128, force_all_rays=False, noises=nz)
        assert x.shape[0] == M and counter == [total, N]
        np.testing.assert_array_equal(r[:, [0, 2]], rr[:, [0, 2]])          # ray ids and sample counts do not depend on the layout
        rot = min(int(np.float32(frac) * np.float32(N)), N - 1)
        order = np.concatenate([np.arange(rot, N), np.arange(0, rot)])      # the scan order
        np.testing.assert_array_equal(r[order, 1], np.concatenate([[0], np.cumsum(rr[order, 2])[:-1]]))
        kept = (r[:, 1] + r[:, 2]) <= M
        assert (~kept).any() and kept[rot] == (rr[rot, 2] <= M)
        assert np.all(np.diff(kept[order].astype(np.int32)) <= 0)           # in scan order: a kept prefix, then the dropped run
        if frac == 0.93:
            assert kept[N - 1] and not kept[rot - 1]                        # the dropped run ends just before the rotation point, not at the last ray
        for n in np.nonzero(kept & (rr[:, 2] > 0))[0][::37]:                  # kept rays hold the exact-size march's samples, bit for bit
            np.testing.assert_array_equal(x[r[n, 1]:r[n, 1] + r[n, 2]], xr[rr[n, 1]:rr[n, 1] + rr[n, 2]])
            np.testing.assert_array_equal(l[r[n, 1]:r[n, 1] + r[n, 2]], lr[rr[n, 1]:rr[n, 1] + rr[n, 2]])
        for n in np.nonzero(~kept)[0][::37]:                                # nothing is written for a dropped ray
            lo, hi = min(r[n, 1], M), min(r[n, 1] + r[n, 2], M)
            assert not x[lo:hi].any() and not l[lo:hi].any()
    # a budget that is large enough: plain ray order whatever the jitter draw
    Mbig = (total + 1023) // 128 * 128
    got = gpu_march(rm, bound, H, dt_gamma, max_steps, mean_count=Mbig - 128, force_all_rays=False, noises=nz)
    np.testing.assert_array_equal(got[3], rr)
    np.testing.assert_array_equal(got[0][:total], xr[:total])


@pytest.mark.parametrize("N", [1, 3, 5, 63, 65])
def test_march_and_composite_tiny_ragged_counts(rm, N):
    """fewer rays than one workgroup of four waves holds, and counts that fill the last workgroup only in part"""
    bound, H, dt_gamma, max_steps = 4.0, 64, 0.0, 1024
    want = ML.march_oracle(bound, H, dt_gamma, max_steps, N=N)
    xr, dr, lr, rr = want
    assert rr[0, 2] > 64                                                  # also with one ray there is something to march and to composite
    assert_same_march(gpu_march(rm, bound, H, dt_gamma, max_steps, N=N), want, N)
    M = xr.shape[0]
    rng = np.random.default_rng(4)
    sig = (rng.random(M).astype(np.float32) * 3) ** 2
    rgb = rng.random((M, 3)).astype(np.float32)
    ws_ref, dep_ref, img_ref = co.composite_rays_train_forward(sig, rgb, lr, rr, 1e-4)
    s, c = cuda(sig).requires_grad_(True), cuda(rgb).requires_grad_(True)
    ws, dep, img = rm.composite_rays_train(s, c, cuda(lr), cuda(rr), 1e-4)
    assert ws.shape == (N,) and img.shape == (N, 3)
    np.testing.assert_allclose(ws.detach().cpu().numpy(), ws_ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dep.detach().cpu().numpy(), dep_ref, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(img.detach().cpu().numpy(), img_ref, rtol=1e-5, atol=1e-6)
    g_ws = rng.standard_normal(N).astype(np.float32)
    g_img = rng.standard_normal((N, 3)).astype(np.float32)
    gs_ref, gc_ref = co.composite_rays_train_backward(g_ws, g_img, sig, rgb, lr, rr, ws_ref, img_ref, 1e-4)
    torch.autograd.backward([ws, img], [cuda(g_ws), cuda(g_img)])
    np.testing.assert_allclose(s.grad.cpu().numpy(), gs_ref, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(c.grad.cpu().numpy(), gc_ref, rtol=1e-4, atol=1e-6)


def _composite_table_on_gpu(rm, t, stride, M, rays, g_ws, g_img):
    s = cuda(t["sigmas"][:M]).requires_grad_(True)
    c = cuda(t["rgbs"][:M] if stride == 4 else t["rgbs"][:M, :3]).requires_grad_(True)
    ws, dep, img = rm.composite_rays_train(s, c, cuda(t["deltas"][:M]), cuda(rays), ML.TABLE_T_THRESH)
    torch.autograd.backward([ws, img], [cuda(g_ws), cuda(g_img)])
    return [a.detach().cpu().numpy() for a in (ws, dep, img, s.grad, c.grad)]


@pytest.mark.parametrize("dropped_tail", [False, True], ids=["whole", "last_ray_over_budget"])
@pytest.mark.parametrize("stride", [3, 4])
def test_composite_table_vs_float64(rm, stride, dropped_tail):
    """The wave kernels carry T, t and the colour sums across chunks of 64 samples and stop at the chunk after which T < T_thresh; the table
    puts ray ends and that crossing before, on and after the boundary.  Against the float64 serial loop at the tolerances the project holds
    this kernel to elsewhere (the float32 C oracle is within 4.2e-7 absolute of float64 on this table and meets them,
    test_composite_table_holds_what_the_gpu_test_relies_on).  `last_ray_over_budget`: the sample arrays end 10 rows before ray 13 does."""
    t = ML.composite_table()
    rays = t["rays"]
    M = t["sigmas"].shape[0] - (10 if dropped_tail else 0)
    f = ML.composite_train_f64(t["sigmas"][:M], t["rgbs"][:M], t["deltas"][:M], rays, ML.TABLE_T_THRESH, t["grad_ws"], t["grad_image"])
    assert f["margin"] > 1                                                # no keep decision can flip through rounding
    ws, dep, img, gs, gc = _composite_table_on_gpu(rm, t, stride, M, rays, t["grad_ws"], t["grad_image"])
    np.testing.assert_allclose(ws, f["ws"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(img, f["image"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dep, f["depth"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(gs, f["grad_sigmas"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(gc[:, :3], f["grad_rgbs"], rtol=1e-4, atol=1e-6)
    slot = rays[:, 0]
    # outputs land in slot rays[n, 0]: the same rays with the identity table give, ray by ray, the same bits (and read their gradients there)
    ident = rays.copy()
    ident[:, 0] = np.arange(rays.shape[0])
    ws_i, dep_i, img_i, gs_i, gc_i = _composite_table_on_gpu(rm, t, stride, M, ident, t["grad_ws"][slot], t["grad_image"][slot])
    for a, b in ((ws, ws_i), (dep, dep_i), (img, img_i)):
        np.testing.assert_array_equal(a[slot], b)
    np.testing.assert_array_equal(gs, gs_i)
    np.testing.assert_array_equal(gc, gc_i)
    live = np.ones(rays.shape[0], bool)
    live[0] = False
    if dropped_tail:
        live[13] = False
        assert not gs[rays[13, 1]:].any() and not gc[rays[13, 1]:].any()
    else:
        assert ws[slot[13]] == 1.0 and img[slot[13]].tolist() == t["rgbs"][rays[13, 1] + 100, :3].tolist()     # alpha == 1 exactly, T == 1 before
    for a in (ws, dep, img):
        assert not a[slot[~live]].any() and np.all(a[slot[live]] > 0)     # no samples or over budget: zeros
    assert np.all(gs[~f["kept"]] == 0) and np.all(gc[~f["kept"]] == 0)    # nothing behind the sample at which the serial loop breaks
    for n in ML.TABLE_OPAQUE:
        off, ln = rays[n, 1], rays[n, 2]
        assert (~f["kept"][off:off + ln]).any() and np.all(gc[off:off + ln][f["kept"][off:off + ln], :3].sum(axis=1) != 0)
    off = rays[13, 1]
    assert np.isfinite(gs[off:]).all() and np.isfinite(gc[off:]).all() and np.isfinite([ws[slot[13]], dep[slot[13]]]).all()
    if stride == 4:
        assert np.all(gc[:, 3] == 0)


def test_inference_loop_three_cascades(rm):
    """the alive-list loop of test_inference_march_composite_compact on 997 rays, three cascades, dt_gamma = 1/64 and 4-channel colours"""
    bound, H = 4.0, 64
    case = ML.march_case(bound, H)
    C, o, d, bitfield, nears, fars = case["C"], case["o"], case["d"], case["bitfield"], case["nears"], case["fars"]
    N = ML.N_RAYS
    rng = np.random.default_rng(5)

    def field(xyz):                       # closed-form sigma / rgb so both sides evaluate the same numbers
        s = 40.0 * np.exp(-(xyz ** 2).sum(-1) / 2.4).astype(np.float32)
        c = (0.5 + 0.5 * np.sin(xyz * 3.0)).astype(np.float32)
        return s, c

    ws_r, dep_r, img_r = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros((N, 3), np.float32)
    alive_r, t_r = np.arange(N, dtype=np.int32), nears.copy()
    ws, dep, img = torch.zeros(N).cuda(), torch.zeros(N).cuda(), torch.zeros(N, 3).cuda()
    alive, t = torch.arange(N, dtype=torch.int32).cuda(), cuda(nears)
    alive_next = torch.empty_like(alive)
    count = torch.zeros(1, dtype=torch.int32).cuda()
    o_g, d_g, bf_g, n_g, f_g = cuda(o), cuda(d), cuda(bitfield), cuda(nears), cuda(fars)
    step, iters, by_threshold = 0, 0, 0
    while step < 1024:
        n_alive = alive_r.shape[0]
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        noises = rng.random(n_alive).astype(np.float32) if step == 0 else np.zeros(n_alive, np.float32)
        xr, dr, lr = co.march_rays(n_alive, n_step, alive_r, t_r, o, d, bound, bitfield, C, H, nears, fars, 128, noises, 1.0 / 64, 1024)
        x, dd, l = rm.march_rays(n_alive, n_step, alive, t, o_g, d_g, bound, bf_g, C, H, n_g, f_g, 128, False, 1.0 / 64, 1024, noises=cuda(noises))
        np.testing.assert_array_equal(x.cpu().numpy(), xr)
        np.testing.assert_array_equal(dd.cpu().numpy(), dr)
        np.testing.assert_array_equal(l.cpu().numpy(), lr)
        s_np, c_np = field(xr)
        c4 = np.concatenate([c_np, rng.random((c_np.shape[0], 1)).astype(np.float32)], axis=1)
        co.composite_rays(n_alive, n_step, alive_r, t_r, s_np, c_np, lr, ws_r, dep_r, img_r, 1e-2)
        rm.composite_rays(n_alive, n_step, alive, t, cuda(s_np), cuda(c4), l, ws, dep, img, 1e-2)
        by_threshold += int(((alive_r < 0) & (lr[:n_alive * n_step].reshape(n_alive, n_step, 2)[:, -1, 0] != 0)).sum())
        alive_r = np.ascontiguousarray(alive_r[alive_r >= 0])
        rm.compact_rays_alive(alive, n_alive, alive_next, count)
        alive, alive_next = alive_next, alive
        k = int(count.item())
        assert k == alive_r.shape[0]
        np.testing.assert_array_equal(alive[:k].cpu().numpy(), alive_r)          # order-preserving, exact
        step += n_step
        iters += 1
    assert iters > 5 and by_threshold > 20                                # rays end at the box and rays end opaque
    # __expf (device fast intrinsic) vs expf: ~1e-6 per sample, accumulated over the ray; budget 1e-5 (north_star: 1e-4)
    np.testing.assert_allclose(ws.cpu().numpy(), ws_r, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(img.cpu().numpy(), img_r, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(dep.cpu().numpy(), dep_r, rtol=1e-5, atol=5e-5)
    np.testing.assert_array_equal(t.cpu().numpy(), t_r)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3000])
def test_compact_rays_alive_tile_edges(rm, n):
    """the compaction tiles by 1024 with a running base: lengths on and next to a wave and a tile, every survivor pattern"""
    rng = np.random.default_rng(n)
    ids = rng.permutation(n + 7)[:n].astype(np.int32)                     # ray ids: distinct, unordered, not the positions
    patterns = dict(all_alive=np.ones(n, bool), all_dead=np.zeros(n, bool), alternating=np.arange(n) % 2 == 0, random=rng.random(n) < 0.4)
    for name, alive in patterns.items():
        a = np.where(alive, ids, -1).astype(np.int32)
        pad = np.concatenate([a, np.arange(5, dtype=np.int32)])          # entries past n are not part of the list
        out = torch.full((n + 5,), -7, dtype=torch.int32).cuda()
        count = torch.full((1,), -7, dtype=torch.int32).cuda()
        rm.compact_rays_alive(cuda(pad), n, out, count)
        want = a[a >= 0]
        assert int(count.item()) == want.shape[0], name
        out = out.cpu().numpy()
        np.testing.assert_array_equal(out[:want.shape[0]], want, err_msg=name)
        assert np.all(out[want.shape[0]:] == -7), name                    # nothing written past the survivors


def test_morton_to_the_abi_limit_and_packbits_special_cells(rm):
    rng = np.random.default_rng(0)
    coords = rng.integers(0, 1024, size=(5000, 3)).astype(np.int32)
    coords[:4] = [[1023, 1023, 1023], [0, 0, 1023], [1023, 0, 0], [512, 1023, 511]]
    idx = rm.morton3D(cuda(coords)).cpu().numpy()
    np.testing.assert_array_equal(idx, co.morton3D(coords))
    assert idx[0] == 0x3FFFFFFF and idx[1] == 0x24924924
    back = rm.morton3D_invert(cuda(idx)).cpu().numpy()
    np.testing.assert_array_equal(back, coords)
    np.testing.assert_array_equal(back, co.morton3D_invert(idx))
    # C = 3, H = 8: 192 bytes, less than one workgroup; cells at the threshold, invalid (-1) and NaN are not occupied
    thresh = np.float32(0.37)
    grid = rng.random((3, 8 ** 3)).astype(np.float32)
    kind = np.arange(8 ** 3) % 9                                          # 0-3: the special cells below, the rest random; 9 and 8 are coprime
    grid[:, kind == 0] = thresh
    grid[:, kind == 1] = -1.0
    grid[:, kind == 2] = np.nan
    grid[:, kind == 3] = np.nextafter(thresh, np.float32(1))
    want = co.packbits(grid, float(thresh))
    bits = np.unpackbits(want, bitorder="little").reshape(3, -1)
    assert want.shape == (192,) and not bits[:, kind <= 2].any() and bits[:, kind == 3].all() and 0.4 < bits[:, kind > 3].mean() < 0.8
    np.testing.assert_array_equal(rm.packbits(cuda(grid), float(thresh)).cpu().numpy(), want)


def test_update_extra_state_three_cascades():
    """test_update_extra_state_kernels_vs_oracle with bound 4: the third cascade's cells span +-4 (csrc/occupancy.hip)"""
    import oracle.torch_oracle as to
    from test_gpu_render import _fields
    model, ref, opt = _fields(cuda_ray=True, bound=4.0)
    assert model.cascade == 3
    Hs = 32
    model.grid_size = Hs
    model.density_grid = torch.zeros(model.cascade, Hs ** 3, device='cuda')
    model.density_bitfield = torch.zeros(model.cascade * Hs ** 3 // 8, dtype=torch.uint8, device='cuda')
    model.density_grid[2, 77] = -1.0                                  # an invalid cell stays untouched and out of the mean
    grid_ref = model.density_grid.cpu().numpy()
    gen = torch.Generator().manual_seed(4)
    for it in range(2):
        rand = [torch.rand(Hs ** 3, 3, generator=gen) for _ in range(model.cascade)]
        model.local_step = 0
        model.update_extra_state(_rand=rand)
        grid_ref, mean_ref, bits_ref = to.update_extra_state(ref, grid_ref, opt.bound, model.cascade, Hs, 0.95, opt.density_thresh, rand)
        dg = model.density_grid.cpu().numpy()
        assert dg[2, 77] == -1.0
        np.testing.assert_allclose(dg, grid_ref, rtol=2e-4, atol=1e-5)
        np.testing.assert_allclose(model.mean_density, mean_ref, rtol=1e-4)
        bits = model.density_bitfield.cpu().numpy()
        assert np.unpackbits(bits ^ bits_ref).sum() <= 4              # cells within rounding of the threshold may differ
        np.testing.assert_array_equal(bits, co.packbits(dg, min(model.mean_density, model.density_thresh)))
        assert all(np.unpackbits(bits_ref.reshape(3, -1)[cas]).sum() > 0 for cas in range(3))
    assert model.iter_density == 2
