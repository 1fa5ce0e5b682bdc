"""Inputs of tests/test_gpu_run_shapes.py, built on the CPU from fixed seeds so that tests/test_run_restatement_host.py can check, without a
GPU, what the GPU tests assume about them (every ray class is there; ill-conditioned inverse-CDF draws stay under their cap)."""
import numpy as np
import torch

FLT_MAX = float(np.finfo(np.float32).max)
MIN_NEAR = 0.01
BOUNDS = (2.0, 1.3)
RAY_CLASSES = ("outside", "inside", "miss", "behind", "nan_near", "axis_parallel")
SIGMA_CLASSES = ("random", "zero", "spike", "inf", "nan")

MERGE_TT = [(3, 2), (4, 3), (16, 48), (63, 5), (64, 64), (65, 63), (100, 7), (128, 127), (128, 128)]
MERGE_N = [1, 3, 4, 5, 64]
PDF_BINS = [2, 3, 64, 65, 66, 256]
PDF_SAMPLES = [1, 2, 63, 64, 65, 200]
PDF_B = [1, 5]
COARSE_T = [2, 3, 63, 64, 65, 127, 128]
COARSE_N = [1, 5, 1000]
COMPOSITE_S = [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256]
FLUSH_TT = [(32, 32), (64, 64), (96, 32), (32, 96), (128, 128)]
RECON_N = [1, 255, 256, 257, 16384, 16385, 40000]


def aabb_of(bound):
    return torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32)


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def make_rays(bound, n_per, seed=0):
    """-> o, d [6 * n_per, 3] float32 and the intended class of every row (index into RAY_CLASSES); rows interleave the classes, so that
    any six consecutive rows hold all of them"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    b = float(np.float32(bound))
    inner = (r(n_per, 3) * 2 - 1) * 0.5 * b
    out_o = _unit(torch.randn(n_per, 3, generator=g)) * 1.9 * b * (1 + 0.2 * r(n_per, 1))
    toward = _unit(inner - out_o)
    rays = {}
    rays["outside"] = (out_o, toward)
    rays["inside"] = ((r(n_per, 3) * 2 - 1) * 0.8 * b, _unit(torch.randn(n_per, 3, generator=g)))
    miss_o = torch.cat([torch.full((n_per, 1), 3 * b), (r(n_per, 2) * 2 - 1) * 0.5 * b], -1)
    rays["miss"] = (miss_o, _unit(torch.tensor([0.1, 1.0, 0.3]) + 0.05 * r(n_per, 3)))
    rays["behind"] = (out_o.clone(), -toward)                              # looking away from the box: the slab intervals lie behind the origin
    nan_o = (r(n_per, 3) * 2 - 1) * 0.6 * b
    nan_o[:, 0] = -b                                                       # on the x = -bound plane, with no x component: (aabb - o) / d = 0 * inf
    nan_d = torch.randn(n_per, 3, generator=g)
    nan_d[:, 0] = 0.0
    rays["nan_near"] = (nan_o, _unit(nan_d))
    ax_o = torch.stack([0.3 * b * (r(n_per) * 2 - 1), torch.full((n_per,), -3 * b), 0.4 * b * (r(n_per) * 2 - 1)], -1)
    ax_d = torch.zeros(n_per, 3)
    ax_d[:, 1] = 1.0
    rays["axis_parallel"] = (ax_o, ax_d)
    o = torch.stack([rays[k][0] for k in RAY_CLASSES], 1).reshape(-1, 3).float().contiguous()
    d = torch.stack([rays[k][1] for k in RAY_CLASSES], 1).reshape(-1, 3).float().contiguous()
    cls = torch.arange(6).repeat(n_per)
    return o, d, cls


def classify(nears, fars):
    """the class near_far_from_aabb's answer puts a ray in: 'nan', 'miss', 'behind' (far < near) or 'valid'"""
    nears, fars = torch.as_tensor(nears).cpu().double(), torch.as_tensor(fars).cpu().double()
    out = np.full(nears.shape[0], "valid", dtype=object)
    out[((fars < nears)).numpy()] = "behind"
    out[(nears == FLT_MAX).numpy()] = "miss"
    out[(torch.isnan(nears) | torch.isnan(fars)).numpy()] = "nan"
    return out


def assert_ray_classes(cls, nears, fars):
    """every intended class came out of near_far_from_aabb as what it was built to be, and none is empty"""
    got = classify(nears, fars)
    want = {"outside": "valid", "inside": "valid", "miss": "miss", "behind": "behind", "nan_near": "nan", "axis_parallel": "valid"}
    for k, name in enumerate(RAY_CLASSES):
        rows = (cls == k).numpy()
        assert rows.any(), name
        assert (got[rows] == want[name]).all(), (name, got[rows])


def make_sigma(N, T, seed=0):
    """[N, T] float32: row n is of class SIGMA_CLASSES[(n // 6) % 5] (with make_rays' interleaving every ray class meets every sigma class
    within 30 rows).  Rays turn opaque along the way, but not by their random first sample: the pdf is over weights[1:-1], so behind an
    opaque sample 0 it is the 1e-5 floor plus dust whose float32 rounding (6e-8 absolute, in `1 - alpha + 1e-15`) is 1e-3 of the total —
    the float32 oracle itself is then 150 bounds away from float64, and the fine-sample bound, which models the CDF arithmetic, says
    nothing about it.  (A spike or an inf ON sample 0 leaves 1e-15 exactly, in either precision.)"""
    g = torch.Generator().manual_seed(2000 + seed)
    s = (torch.rand(N, T, generator=g) * 5) ** 2
    s[:, 0] *= 0.01
    where = torch.randint(0, T, (N,), generator=g)
    for n in range(N):
        k = SIGMA_CLASSES[(n // 6) % 5]
        if k == "zero":
            s[n] = 0
        elif k == "spike":
            s[n] *= 0.01
            s[n, where[n]] = 1e4
        elif k == "inf":
            s[n, where[n]] = float("inf")
        elif k == "nan":
            s[n, where[n]] = float("nan")
    return s


def make_u(N, t, seed=0):
    """[N, t] float32 draws with repeated values in every row (ties among the fine samples)"""
    g = torch.Generator().manual_seed(3000 + seed)
    u = torch.rand(N, t, generator=g)
    u[:, 1] = u[:, 0]
    u[::2, -1] = u[::2, 0]
    return u


def merge_cases():
    """(T, t, N, det, bound, first row, seed) of every configuration of the merge tests.  N rows are taken from a 66-ray batch from `first`
    on, which moves with the configuration, so that N = 1 meets every ray class"""
    out = []
    for T, t in MERGE_TT:
        for N in MERGE_N:
            for det in (False, True):
                for bound in BOUNDS:
                    k = len(out)
                    out.append((T, t, N, det, bound, 0 if N == 64 else k % 30, k))
    return out


def merge_inputs(case):
    """-> o, d [N, 3], cls [N], noise [N, T], sigma [N, T], u [N, t] or None, all float32 CPU tensors"""
    T, t, N, det, bound, first, seed = case
    o, d, cls = make_rays(bound, 11, seed=int(bound * 10))
    o, d, cls = o[first:first + N].contiguous(), d[first:first + N].contiguous(), cls[first:first + N]
    noise = torch.rand(N, T, generator=torch.Generator().manual_seed(4000 + seed))
    sigma = make_sigma(66, T, seed)[first:first + N].contiguous()
    return o, d, cls, noise, sigma, (None if det else make_u(N, t, seed))


def coarse_f32(o, d, nears, fars, aabb, T, noise):
    """the coarse samples as the float32 oracle forms them (oracle.torch_oracle.run): the CPU stand-in for k_sample_coarse's z"""
    nears, fars = torch.as_tensor(nears).reshape(-1, 1), torch.as_tensor(fars).reshape(-1, 1)
    z = nears + (fars - nears) * torch.linspace(0.0, 1.0, T)[None]
    return z + (noise - 0.5) * ((fars - nears) / T)


def pdf_inputs(n_bins, B, kind, seed=0):
    """bins [B, n_bins] ascending, weights [B, n_bins - 1]: kind 'zero' (all-zero weights) or 'spike' (small random weights, one of 50)"""
    g = torch.Generator().manual_seed(5000 + 7 * n_bins + B + seed)
    bins = torch.sort(torch.rand(B, n_bins, generator=g) * 3 + 0.2, dim=-1).values
    w = torch.zeros(B, n_bins - 1)
    if kind == "spike":
        w = torch.rand(B, n_bins - 1, generator=g) * 0.02
        w[torch.arange(B), torch.randint(0, n_bins - 1, (B,), generator=g)] = 50.0
    return bins, w


def pdf_u(B, n_samples, seed=0):
    return torch.rand(B, n_samples, generator=torch.Generator().manual_seed(6000 + 13 * n_samples + B + seed))


COMPOSITE_ROWS = ("random", "zero_sigma", "opaque_first", "descending_z", "missed")


def composite_inputs(N, S, first=0, seed=0, exact_half_conf=False):
    """-> sigma [N, S], rgbc [N, S, 4], z [N, S], nears, fars [N] (float32 CPU); row n is of kind COMPOSITE_ROWS[(first + n) % 5].
    The descending row keeps sigma under 0.1, so that its growing 'transmittance' exp(sum |delta| sigma) and with it the outputs stay of the
    order of one, where the forward's absolute tolerance means what it means for the other rows."""
    g = torch.Generator().manual_seed(7000 + 31 * S + seed)
    sig = (torch.rand(N, S, generator=g) * 6) ** 2
    rgbc = torch.rand(N, S, 4, generator=g)
    if exact_half_conf:
        rgbc[:, ::3, 3] = 0.5
    z = torch.sort(torch.rand(N, S, generator=g) * 3 + 0.3, dim=-1).values
    nears, fars = z[:, 0] - 0.05, z[:, -1] + 0.2
    for n in range(N):
        k = COMPOSITE_ROWS[(first + n) % 5]
        if k == "zero_sigma":
            sig[n] = 0
        elif k == "opaque_first":
            sig[n, 0] = 1e4
        elif k == "descending_z":
            z[n] = z[n].flip(0)
            sig[n] = sig[n] / 360
            nears[n], fars[n] = z[n, 0] + 0.05, z[n, -1] - 0.2
        elif k == "missed":
            z[n] = FLT_MAX
            nears[n] = fars[n] = FLT_MAX
    return sig.contiguous(), rgbc.contiguous(), z.contiguous(), nears.contiguous(), fars.contiguous()


def is_row_permutation(src, N, T, t):
    """src [N, T + t] int: row n holds each of n*T .. n*T+T-1 and N*T+n*t .. N*T+n*t+t-1 exactly once"""
    src = np.asarray(torch.as_tensor(src).cpu().numpy()).astype(np.int64) & 0xFFFFFFFF
    n = np.arange(N)[:, None]
    want = np.concatenate([n * T + np.arange(T)[None], N * T + n * t + np.arange(t)[None]], 1)
    return np.array_equal(np.sort(src, 1), want)


def in_sort_order(z):
    """z [N, S] float: every row ascending with its NaNs last (torch.sort's order)"""
    z = torch.as_tensor(z).cpu().double()
    nan = torch.isnan(z)
    nan_last = bool((nan[:, 1:] | ~nan[:, :-1]).all())                     # no number after a NaN
    both = ~nan[:, 1:] & ~nan[:, :-1]
    return nan_last and bool((z[:, 1:] >= z[:, :-1])[both].all())
