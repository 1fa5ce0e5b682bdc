"""k_field_bwd_x2 at the sizes where its software pipeline changes shape: one tile, a ragged last tile, one window more than a full round of
the launch (the tile sets with even and odd step index alternate: a tile's activation images are published one step ahead of its backward,
while the other set's backward still reads its own), and dead windows between live ones (early-termination flags).  fp16, 16 levels x 2
features (feature width 32), two hidden layers, against autograd on the oracle field at the tolerances of tests/test_gpu_field.py; every case
twice, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_oracle as to      # noqa: E402

L, N_GEO = 16, 2
TILE = 32
X2_BLOCKS = 256                            # workgroups of a full k_field_bwd_x2 launch (x2_launch), two tiles per workgroup and window
WINDOW = 2 * TILE * X2_BLOCKS              # samples of one window = one step of every pipeline of the launch


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _live_dead_live():
    """window 0 live (with a few dead single tiles and dead tile pairs inside it: a dead tile beside a live one is processed, a dead pair whose
    window lives too), window 1 dead, window 2 live"""
    t = np.arange(3 * WINDOW // TILE)
    live = (t // (2 * X2_BLOCKS)) != 1
    live &= ~((t < 64) & (t % 2 == 1))
    live &= ~((t >= 128) & (t < 192) & ((t // 2) % 2 == 1))
    return live.astype(np.uint8)


CASES = {
    "one_tile": (TILE, None),
    "ragged_tile": (TILE + 1, None),
    "full_round_plus_one_window": (WINDOW + TILE, None),
    "live_dead_live": (3 * WINDOW, _live_dead_live()),
}


def _case(P, live, seed=21):
    from customnerf_amd.gridencoder import GridEncoder
    ref = to.FieldRef(bound=2.0, num_levels=L, n_hidden_geo=N_GEO, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        ref.pos_en.embeddings.copy_((torch.rand(ref.pos_en.embeddings.shape, generator=g) * 2 - 1) * 0.5)
    ref.half = True
    ref.pos_en.half = True
    enc = GridEncoder(num_levels=L, log2_hashmap_size=19, desired_resolution=2048, gridtype='hash').cuda()
    with torch.no_grad():
        enc.embeddings.copy_(ref.pos_en.embeddings.cuda())
    rng = np.random.default_rng(seed)
    x = ((rng.random((P, 3)) * 2 - 1) * 1.9).astype(np.float32)
    x[:5] *= 0.05                                     # inside the gaussian density blob
    d = rng.standard_normal((P, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    gs = (rng.standard_normal(P) * 0.05).astype(np.float32)
    gc = rng.standard_normal((P, 4)).astype(np.float32)
    if live is not None:                              # a dead tile: every output gradient of its rows is exactly zero
        rows = np.repeat(live, TILE).astype(np.float32)
        gs *= rows
        gc *= rows[:, None]
    return ref, enc, x, d, gs, gc


def _launch(ref, enc, x, d, gs, gc, live, poison_workspace):
    """field forward + backward; with `live` the flags travel the way the compositing backward hands them over (an attribute of the gradient
    tensor); returns what the kernel wrote — the three parameter gradients and d(loss)/d(grid features) — and whether the flags reached it"""
    from customnerf_amd import field as fld
    pn, pd, pr = (t.detach().clone().cuda().requires_grad_(True) for t in (ref.network, ref.density_network, ref.rgb_network))
    with torch.no_grad():
        e = enc.encode(cuda(x), bound=2.0, half=True)
    e.requires_grad_(True)
    s, c = fld.field(e, cuda(x), cuda(d), 1, 2 * L, N_GEO, 4, pn, pd, pr)
    g_s, g_c = cuda(gs), cuda(gc)
    if live is not None:
        g_s._cnerf_tile_live = (cuda(live), g_s.data_ptr(), g_s._version, g_c.data_ptr(), g_c._version)
    if poison_workspace:
        assert fld._WS
        for buf in fld._WS.values():
            buf.fill_(0xFF)
    seen = []
    entry = fld.lib.cnerf_field_backward_img

    def spy(*a):
        seen.append(a[-3] is not None)                # (..., tile_live, weight_image, stream)
        return entry(*a)
    fld.lib.cnerf_field_backward_img = spy
    try:
        torch.autograd.backward([s, c], [g_s, g_c])
    finally:
        fld.lib.cnerf_field_backward_img = entry
    assert len(seen) == 1
    return (pn.grad.clone(), pd.grad.clone(), pr.grad.clone(), e.grad.clone()), seen[0]


def _table_gradient(enc, x, g_enc):
    """the feature gradients scattered into the table (the scatter is not under test: small lists take its atomic form, whose float sums have
    no fixed order — bit identity is asserted on the field kernel's own outputs)"""
    enc.embeddings.grad = None
    e = enc.encode(cuda(x), bound=2.0, half=True)
    e.backward(g_enc)
    return enc.embeddings.grad.clone()


@pytest.mark.parametrize("name", list(CASES))
def test_field_backward_chain(name):
    P, live = CASES[name]
    ref, enc, x, d, gs, gc = _case(P, live)
    s_ref, c_ref, _ = ref(torch.from_numpy(x), torch.from_numpy(d))
    torch.autograd.backward([s_ref, c_ref], [torch.from_numpy(gs), torch.from_numpy(gc)])
    first, flagged = _launch(ref, enc, x, d, gs, gc, live, False)
    assert flagged == (live is not None)
    rt, at = 3e-2, 3e-3                               # test_gpu_field.py::test_field_backward, fp16
    for nm, a, b in zip(("net", "den", "rgb", "grid"), first[:3] + (_table_gradient(enc, x, first[3]),),
                        (ref.network.grad, ref.density_network.grad, ref.rgb_network.grad, ref.pos_en.embeddings.grad)):
        a, b = a.cpu().numpy(), b.numpy()
        scale = float(np.abs(b).max())
        assert scale > 0, nm
        err = np.abs(a - b).max() / scale
        print(f"{name} {nm}: max|diff|/max|ref| = {err:.3e}")
        assert err < (rt if nm != "grid" else rt * 2), f"{nm}: max|diff|/max|ref| = {err:.3e}"
        np.testing.assert_allclose(a, b, rtol=rt * 10, atol=max(at, rt * scale), err_msg=nm)
    pd_g, pr_g = first[1], first[2]
    assert torch.all(pd_g[4096 + 64:] == 0)          # padded parameter rows / columns get exactly zero
    assert torch.all(pr_g[:64 * 96].view(64, 96)[:, 91:] == 0)
    # the second launch from a workspace of 0xFF bytes: same bits
    second, _ = _launch(ref, enc, x, d, gs, gc, live, True)
    for a, b in zip(first, second):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a, b)
    if live is not None:                              # and the flags change nothing: dead tiles contribute exact zeros either way
        plain, flagged = _launch(ref, enc, x, d, gs, gc, None, False)
        assert not flagged
        for a, b in zip(first, plain):
            assert torch.equal(a, b)
