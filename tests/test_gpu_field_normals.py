"""GPU: the field-normal kernels (customnerf_amd/csrc/field_normal.hip) and the surface built on them, against the float64 restatement
(tests/field_normal_restatement.py) and the oracle field (oracle/torch_oracle.py FieldRef)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import field_normal_restatement as FN  # noqa: E402
import tsdf_restatement as T  # noqa: E402
from mesh_testlib import AABB, dtype_guard, gaussian_model  # noqa: E402,F401
from oracle import torch_oracle as to  # noqa: E402

CONFIGS = [(16, 2), (4, 1), (17, 1), (32, 2)]             # the four dispatch classes (enc_pad / 16 = 2, 1, 3, 4)
SIZES = (1, 33, 2049)                                     # ragged against the 32-sample tile
P_MAX = SIZES[-1]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(L, n_geo, gridtype='hash', seed=0):
    """tests/test_gpu_field.py's make_case: the oracle field with a U(+-0.5) table (hash, log2 T = 19, 2048 finest), the encoder holding
    the same table, P_MAX points of which the first five lie inside the density blob.  Built once per configuration."""
    from customnerf_amd.gridencoder import GridEncoder
    ref = to.FieldRef(bound=2.0, num_levels=L, n_hidden_geo=n_geo, gridtype=gridtype, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        ref.pos_en.embeddings.copy_((torch.rand(ref.pos_en.embeddings.shape, generator=g) * 2 - 1) * 0.5)
    enc = GridEncoder(num_levels=L, log2_hashmap_size=19, desired_resolution=2048, gridtype=gridtype).cuda()
    with torch.no_grad():
        enc.embeddings.copy_(ref.pos_en.embeddings.cuda())
    rng = np.random.default_rng(seed)
    x = ((rng.random((P_MAX, 3)) * 2 - 1) * 1.9).astype(np.float32)
    x[:5] *= 0.05
    return ref, enc, x


@functools.lru_cache(maxsize=None)
def features(L, n_geo, half):
    """(enc [L, P_MAX, 2] on the device in the kernel layout, the same as [P_MAX, 2 L] float32 on the host)"""
    ref, enc, x = case(L, n_geo)
    with torch.no_grad():
        e = enc.encode(cuda(x), bound=2.0, half=half)
    return e, e.float().permute(1, 0, 2).reshape(P_MAX, 2 * L).cpu()


# ------------------------------------------------------------------------------------------------ the forward inside the gradient kernel
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("L,n_geo", CONFIGS)
def test_same_forward(L, n_geo, half):
    """sigma of cnerf_field_density_grad is the forward kernel's, bit for bit, at every ragged size; grad_enc does not depend on P"""
    from customnerf_amd.field import field_density_grad, field_forward_raw
    ref, _, x = case(L, n_geo)
    e, _ = features(L, n_geo, half)
    pn, pd = ref.network.detach().cuda(), ref.density_network.detach().cuda()
    full = None
    for P in reversed(SIZES):
        xs = cuda(x[:P])
        want, _ = field_forward_raw(e, xs, None, 1, 2 * L, n_geo, 4, pn, pd, None, with_rgb=False)
        sigma, g = field_density_grad(e, xs, 2 * L, n_geo, pn, pd)
        assert torch.equal(sigma, want), P
        assert tuple(g.shape) == (L, P, 2) and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        none, g2 = field_density_grad(e, xs, 2 * L, n_geo, pn, pd, want_sigma=False)
        assert none is None and torch.equal(g2, g)
        full = g if full is None else full
        assert torch.equal(g, full[:, :P])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_level_stride_and_row_offset(half):
    """rows 100 .. 100 + 333 of a feature buffer with 2049 rows per level, handed over as a flat view that starts at row 100"""
    from customnerf_amd.field import field_density_grad
    L, n_geo, row0, P = 16, 2, 100, 333
    ref, _, x = case(L, n_geo)
    e, _ = features(L, n_geo, half)
    pn, pd = ref.network.detach().cuda(), ref.density_network.detach().cuda()
    s_all, g_all = field_density_grad(e, cuda(x), 2 * L, n_geo, pn, pd)
    s, g = field_density_grad(e.reshape(-1)[row0 * 2:], cuda(x[row0:row0 + P]), 2 * L, n_geo, pn, pd, enc_level_stride=P_MAX)
    assert torch.equal(s, s_all[row0:row0 + P]) and torch.equal(g, g_all[:, row0:row0 + P])


# ------------------------------------------------------------------------------------------------ d raw / d enc
KINK = 1e-5          # samples whose smallest hidden |pre-activation| is below KINK * max |z| sit on a ReLU kink: excluded, at most 5 % of them


@pytest.mark.parametrize("L,n_geo", CONFIGS)
def test_mlp_gradient_fp32(L, n_geo):
    from customnerf_amd.field import field_density_grad
    ref, _, x = case(L, n_geo)
    e, e_host = features(L, n_geo, False)
    _, g = field_density_grad(e, cuda(x), 2 * L, n_geo, ref.network.detach().cuda(), ref.density_network.detach().cuda(), want_sigma=False)
    got = g.permute(1, 0, 2).reshape(P_MAX, 2 * L).cpu().double()
    _, want, margin, zmax = FN.raw_and_grad(e_host, ref.network, ref.density_network, 2 * L, n_geo)
    keep = margin >= KINK * zmax
    share = 1.0 - float(keep.double().mean())
    err = (got - want).abs()[keep]
    tol = (1e-4 * want.abs() + 1e-6 * float(want.abs().max()))[keep]
    print(f"fp32 grad_enc L={L} n_geo={n_geo}: excluded {share:.4f}, max err / max|g| = {float(err.max()) / float(want.abs().max()):.3e}")
    assert share <= 0.05
    assert bool((err <= tol).all()), float((err - tol).max())


@pytest.mark.parametrize("L,n_geo", CONFIGS)
def test_mlp_gradient_fp16(L, n_geo):
    """Relative L2 error per sample of the half-precision kernel against the float64 gradient of the unrounded-activation field with the
    same fp16-rounded weights: median and 90th percentile at most 1.5 x those of the oracle's own half mode (FieldRef(half=True) against
    FieldRef(half=False), as the oracle defines them, on the same features) — a ReLU mask that flips under rounding changes a sample's
    gradient by a finite amount, so no pointwise bound exists; the factor covers the MFMA's summation order.
    Measured on the MI355X, median / 90th percentile, kernel | oracle's half mode:
      L = 16, 2 hidden  3.58e-4 / 4.92e-4 | 6.16e-4 / 8.47e-4        L = 4, 1 hidden   3.49e-4 / 5.84e-4 | 6.10e-4 / 9.95e-4
      L = 17, 1 hidden  2.91e-4 / 3.90e-4 | 5.12e-4 / 6.53e-4        L = 32, 2 hidden  3.52e-4 / 4.72e-4 | 5.80e-4 / 7.54e-4
    (the oracle's figures contain the rounding of the weights, the kernel's only that of the gradient vectors between layers)."""
    from customnerf_amd.field import field_density_grad
    ref, _, x = case(L, n_geo)
    e, e_host = features(L, n_geo, True)
    pn16, pd16 = ref.network.detach().half().float(), ref.density_network.detach().half().float()
    _, g = field_density_grad(e, cuda(x), 2 * L, n_geo, pn16.cuda(), pd16.cuda(), want_sigma=False)
    got = g.permute(1, 0, 2).reshape(P_MAX, 2 * L).cpu().double()
    rel = lambda a, b: ((a.double() - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-300)).numpy()          # noqa: E731
    want = FN.raw_and_grad(e_host, pn16, pd16, 2 * L, n_geo)[1]
    base_ref = FN.raw_and_grad(e_host, ref.network, ref.density_network, 2 * L, n_geo)[1]
    base = FN.raw_and_grad(e_host, ref.network, ref.density_network, 2 * L, n_geo, half=True)[1]
    k, b = rel(got, want), rel(base, base_ref)
    km, k90, bm, b90 = np.median(k), np.percentile(k, 90), np.median(b), np.percentile(b, 90)
    print(f"fp16 grad_enc L={L} n_geo={n_geo}: kernel median {km:.3e} p90 {k90:.3e} | oracle half median {bm:.3e} p90 {b90:.3e}")
    assert km <= 1.5 * bm and k90 <= 1.5 * b90, (km, k90, bm, b90)


# ------------------------------------------------------------------------------------------------ d enc / d x, contracted
def grid_points(scale0):
    rng = np.random.default_rng(11)
    x = rng.random((P_MAX, 3)).astype(np.float32)
    x[0], x[1], x[2], x[3] = (0.0, 0.3, 0.7), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.25, 1.0, 0.0)
    for k in range(4):                                                # grid nodes of the coarsest level
        x[4 + k] = (np.float32((k + 1 - 0.5) / scale0), np.float32((2 * k + 2 - 0.5) / scale0), x[4 + k, 2])
    x[8], x[9], x[10] = (-0.01, 0.5, 0.5), (0.5, 1.0000001, 0.5), (0.5, 0.5, 7.0)          # outside: exactly zero
    return x


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("L,gridtype", [(16, 'hash'), (16, 'tiled'), (32, 'hash'), (5, 'hash')])
def test_grid_input_grad(L, gridtype, half):
    """per component within n_terms x 2^-23 x sum |term| of the float64 restatement, n_terms = 16 L: what a float32 accumulation of that
    many terms can lose, however they are ordered"""
    ref, enc, _ = case(L, 1, gridtype)
    pe = ref.pos_en
    x = grid_points(FN.levels(pe.offsets, pe.per_level_scale, 16)[0][2])
    rng = np.random.default_rng(12)
    for B in (P_MAX, 33, 1):
        g_enc = rng.standard_normal((L, B, 2)).astype(np.float32)
        table = (enc.half_table() if half else enc.embeddings.detach()).float().cpu().double()
        got = enc.input_grad(cuda(x[:B]), cuda(g_enc), half=half)
        again = enc.input_grad(cuda(x[:B]), cuda(g_enc), half=half)
        assert torch.equal(got, again)                                # the same bits on every run
        want, absum = FN.grid_input_grad(torch.from_numpy(x[:B]).double(), table, pe.offsets, pe.per_level_scale, 16, torch.from_numpy(g_enc),
                                         pe.gridtype_id)
        err = (got.cpu().double() - want).abs()
        tol = 16 * L * 2.0 ** -23 * absum
        print(f"input_grad L={L} {gridtype} half={half} B={B}: max err / tol = {float((err / tol.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= tol).all())
        if B > 10:
            assert bool((got[8:11] == 0).all()) and bool((got[:8] != 0).any(-1).all())
    # a strided grad_enc: the rows of a larger buffer
    big = cuda(rng.standard_normal((L, 50, 2)).astype(np.float32))
    assert torch.equal(enc.input_grad(cuda(x[:33]), big, level_stride=50, half=half), enc.input_grad(cuda(x[:33]), big[:, :33].contiguous(), half=half))


def test_grid_input_grad_equals_the_generic_path():
    """GridEncoder's own calc_grad_inputs path (dy_dx materialised, float32) gives the same vector: rtol 1e-5 on top of the float32
    accumulation bound of the two results"""
    L = 16
    ref, enc, _ = case(L, 1)
    pe = ref.pos_en
    rng = np.random.default_rng(13)
    x = rng.random((500, 3)).astype(np.float32)
    g_enc = rng.standard_normal((L, 500, 2)).astype(np.float32)
    got = enc.input_grad(cuda(x), cuda(g_enc), half=False)
    xs = (cuda(x) * 2 - 1).requires_grad_(True)                       # bound 1: unit = (xs + 1) / 2, d unit / d xs = 1 / 2
    out = enc.encode(xs, bound=1, half=False)
    (gx,) = torch.autograd.grad(out, xs, cuda(g_enc))
    unit = ((xs.detach() + 1) / 2).cpu()
    want64, absum = FN.grid_input_grad(unit.double(), enc.embeddings.detach().cpu().double(), pe.offsets, pe.per_level_scale, 16,
                                       torch.from_numpy(g_enc), 0)
    got_u = enc.input_grad(unit.cuda(), cuda(g_enc), half=False)      # at the unit coordinates the generic path saw
    tol = 1e-5 * want64.abs() + 2 * 16 * L * 2.0 ** -23 * absum
    assert bool(((got_u.cpu().double() - 2 * gx.cpu().double()).abs() <= tol).all())
    assert float((got - got_u).abs().max()) <= 1e-2 * float(got.abs().max())


# ------------------------------------------------------------------------------------------------ end to end: grad log sigma
def field_model(L, n_geo, tcnn):
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    tcnn.set_default_dtype(torch.float32)
    ref, _, x = case(L, n_geo)
    model = NeRFNetwork(sc.make_opt(num_levels=L, n_hidden_geo=n_geo)).cuda().eval()
    with torch.no_grad():
        model.pos_en.embeddings.copy_(ref.pos_en.embeddings.cuda())
        model.network.params.copy_(ref.network.cuda())
        model.density_network.params.copy_(ref.density_network.cuda())
    return ref, model, x


@pytest.mark.parametrize("L,n_geo", [(16, 2), (4, 1)])
def test_density_gradient_end_to_end(dtype_guard, L, n_geo):
    ref, model, x = field_model(L, n_geo, dtype_guard)
    P = 1029
    with torch.enable_grad():
        out = model.density_gradient(cuda(x[:P]))
    assert not out['grad'].requires_grad and not out['sigma'].requires_grad
    with torch.no_grad():                                             # (the fused density pass; with grad enabled density() takes the tcnn modules)
        assert torch.equal(out['sigma'], model.density(cuda(x[:P]))['sigma'])
    want, margin, zmax = FN.log_density_grad(ref, torch.from_numpy(x[:P]))
    keep = margin >= KINK * zmax
    share = 1.0 - float(keep.double().mean())
    err = (out['grad'].cpu().double() - want).abs()[keep]
    tol = (1e-4 * want.abs() + 1e-6 * float(want.abs().max()))[keep]
    print(f"grad log sigma L={L}: excluded {share:.4f}, max err / max|g| = {float(err.max()) / float(want.abs().max()):.3e}")
    assert share <= 0.05 and bool(keep[:5].all())                     # the five points inside the blob are compared
    assert bool((err <= tol).all()), float((err - tol).max())
    n = model.normal(cuda(x[:P]))
    assert torch.allclose(n.norm(dim=-1), torch.ones(P, device="cuda"), atol=1e-5)
    assert torch.allclose(n, -out['grad'] / out['grad'].norm(dim=-1, keepdim=True), atol=1e-6)


# ------------------------------------------------------------------------------------------------ the per-ray sums
@pytest.mark.parametrize("indexed", [False, True], ids=["identity", "indexed"])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("S", [6, 128])
def test_composite_normals(S, V, indexed):
    from customnerf_amd.nerf.render_ops import composite_normals
    N = 5
    g = torch.Generator().manual_seed(S + V)
    w = torch.rand(V, N, S, generator=g) / S
    gx = torch.randn(N * S + 7, 3, generator=g) * 3
    gx[::5] = 0                                                       # zero-gradient samples: zero normals
    gx[1] = 1e-11                                                     # |g|^2 = 3e-22 < 1e-20: zero as well
    d = torch.randn(N, 3, generator=g)
    src = None
    if indexed:
        src = torch.stack([torch.randperm(S, generator=g) + n * S for n in range(N)]).int()
        src[0, 0] = N * S + 3                                         # a row beyond the [N, S] block
    nm, orient = composite_normals(w.cuda(), None if src is None else src.cuda(), gx.cuda(), d.cuda())
    nm_ref, orient_ref = FN.composite_normals(w, src, gx, d)
    assert tuple(nm.shape) == (V, N, 3) and tuple(orient.shape) == (V, N)
    assert float((nm.cpu().double() - nm_ref).abs().max()) <= 1e-6 and float((orient.cpu().double() - orient_ref).abs().max()) <= 1e-6
    assert float(orient_ref.max()) > 1e-3 and float(nm_ref.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ run(), render_view(), extract_mesh()
def test_run_normals(dtype_guard):
    """split and merged sample lists give the same normal map; the flag changes no other entry"""
    from customnerf_amd import scene as sc
    from customnerf_amd.nerf.network_grid import NeRFNetwork
    from customnerf_amd.nerf.provider_utils import generate_rays
    dtype_guard.set_default_dtype(torch.float32)
    torch.manual_seed(0)
    opt = sc.make_opt(num_levels=16)
    model = NeRFNetwork(opt).cuda().eval()
    with torch.no_grad():
        model.pos_en.embeddings.uniform_(-0.5, 0.5)
    H = W = 8
    o, d = generate_rays(torch.from_numpy(sc.poses(1)).cuda(), *sc.intrinsics(H, W), H, W, 1.0, 'nerfstudio')
    o, d = o.view(1, H * W, 3), d.view(1, H * W, 3)
    res = {}
    for split in (True, False):
        opt.split_eval = split
        with torch.enable_grad():
            plain = model.run(o, d, num_steps=32, upsample_steps=32)
            res[split] = r = model.run(o, d, num_steps=32, upsample_steps=32, normals=True)
        assert 'normal_map' not in plain and 'orient' not in plain and 'normal' not in plain and 'normal_map' not in plain['fg']
        for k in plain:
            if k in ('fg', 'bg'):
                for kk in plain[k]:
                    assert torch.equal(plain[k][kk], r[k][kk]), (split, k, kk)
            else:
                assert torch.equal(plain[k], r[k]), (split, k)
        assert set(r) - set(plain) == {'normal_map', 'orient', 'normal'}
        for part in (r, r['fg'], r['bg']):
            assert tuple(part['normal_map'].shape) == (1, H * W, 3) and tuple(part['orient'].shape) == (1, H * W)
            assert not part['normal_map'].requires_grad
        assert tuple(r['normal'].shape) == (H * W, 64, 3)
        want = (r['weights'][..., None] * r['normal']).sum(1)
        assert torch.allclose(r['normal_map'].view(-1, 3), want, atol=1e-5)
        assert float(r['normal_map'].abs().max()) > 1e-2
    for part in (lambda r: r, lambda r: r['fg'], lambda r: r['bg']):
        a, b = part(res[True]), part(res[False])
        assert torch.allclose(a['normal_map'], b['normal_map'], rtol=0, atol=1e-5)
        assert torch.allclose(a['orient'], b['orient'], rtol=0, atol=1e-5)
    assert torch.allclose(res[True]['normal'], res[False]['normal'], rtol=0, atol=1e-5)


def test_render_view_normals_and_shading(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    with torch.no_grad():
        model.aabb_infer.copy_(torch.tensor(AABB))
    pose, k, H, W = T.look_at((0.4, -1.1, 1.6)), (27.0, 25.0, 8.0, 7.0), 16, 16
    plain = model.render_view(pose, k, H, W, min_opacity=0.9)
    assert set(plain) == {'image', 'depth', 'opacity'}
    a = 0.25
    light = torch.tensor([0.3, -0.5, 0.8])
    unit = (light / light.norm()).cuda()
    for shading, kw in (('normal', {}), ('lambertian', dict(light_d=light, ambient_ratio=a)), ('textureless', dict(light_d=light, ambient_ratio=a)),
                        ('lambertian', {})):
        r = model.render_view(pose, k, H, W, min_opacity=0.9, shading=shading, **kw)
        assert set(r) == {'image', 'depth', 'opacity', 'normal', 'shaded'}
        for key in ('image', 'depth', 'opacity'):
            assert torch.equal(r[key], plain[key])
        n, hit = r['normal'], r['opacity'] >= 0.9
        assert tuple(n.shape) == (H, W, 3) and tuple(r['shaded'].shape) == (H, W, 3)
        assert bool(hit.any()) and bool((~hit).any())
        assert bool((n[~hit] == 0).all()) and torch.allclose(n[hit].norm(dim=-1), torch.ones(int(hit.sum()), device="cuda"), atol=1e-5)
        if shading == 'normal':
            want = (n + 1) / 2
        elif kw:
            lam = a + (1 - a) * (n @ unit).clamp_min(0)[..., None]
            want = (r['image'] if shading == 'lambertian' else torch.ones_like(r['image'])) * lam
        else:
            want = None                                               # the default light stands at the camera: the blob's near side is lit
            assert bool((r['shaded'] >= 0.1 * r['image'] - 1e-6).all()) and bool((r['shaded'] <= r['image'] + 1e-6).all())
            assert bool((r['shaded'][hit].sum(-1) > 0.1 * r['image'][hit].sum(-1) + 1e-4).any())
        if want is not None:
            assert torch.allclose(r['shaded'], want, atol=1e-6)
    # the blob's normals point away from its centre: against the viewing rays
    r = model.render_view(pose, k, H, W, min_opacity=0.9, normals=True, path=str(tmp_path / "n.png"))
    assert set(r) == {'image', 'depth', 'opacity', 'normal'} and (tmp_path / "n.png").stat().st_size > 100
    eye = torch.tensor(pose[:3, 3]).cuda()
    assert bool(((r['normal'][hit] * eye).sum(-1) > 0).all())


def test_extract_mesh_field_normals(dtype_guard, tmp_path):
    model = gaussian_model(dtype_guard, False)
    with torch.no_grad():
        model.density_network.params.copy_(0.02 * torch.randn(model.density_network.params.shape, generator=torch.Generator().manual_seed(2)))
        model.pos_en.embeddings.uniform_(-0.5, 0.5)
    kw = dict(resolution=32, threshold=10.0, aabb=AABB)
    a = model.extract_mesh(**kw)
    b = model.extract_mesh_normals('field', **kw)
    a2 = model.extract_mesh_normals('mesh', **kw)
    assert set(a2) == set(a) and torch.equal(a2['normals'], a['normals']) and torch.equal(a2['verts'], a['verts'])
    assert 'field_normals' not in a and set(b) - set(a) == {'field_normals'}
    assert torch.equal(a['verts'], b['verts']) and torch.equal(a['faces'], b['faces']) and len(a['faces']) > 100
    n, geo = b['normals'], a['normals']
    fn = model.normal(b['verts'])
    keep = (fn * geo).sum(-1) <= 0
    assert b['field_normals'] == {'kept_geometric': int(keep.sum())}
    assert torch.equal(n[~keep], fn[~keep]) and torch.equal(n[keep], geo[keep])
    assert bool(((n * geo).sum(-1) > 0).all())
    assert torch.allclose(n[~keep].norm(dim=-1), torch.ones(int((~keep).sum()), device="cuda"), atol=1e-5)
    assert int(keep.sum()) < len(n) // 2 and not torch.equal(n, geo)
    for bad in (dict(part='fg'), dict(remesh=16), dict(tsdf=dict(poses=T.sphere_cameras(), intrinsics=T.INTRINSICS, H=T.IMG, W=T.IMG))):
        with pytest.raises(ValueError):
            model.extract_mesh_normals('field', **kw, **bad)
    c = model.save_mesh(str(tmp_path / "m.ply"), normals='field', color=True, **kw)      # the colours look along the field's normals
    assert c['colors'] is not None and torch.equal(c['normals'], n) and (tmp_path / "m.ply").stat().st_size > 1000
