"""Float64 torch restatement of what the field-normal kernels (customnerf_amd/csrc/field_normal.hip) compute, for the tests.

Grid part: the trilinear hash / tiled interpolation of the fused field's configuration (3-D, 2 features per level, linear, no
align_corners), built from oracle.torch_oracle.grid_offsets, the oracle's level geometry (oracle.c_oracle.level_geometry) and the oracle's
index rule (gridencoder.cu:66-84), differentiable in x by autograd, plus the explicit derivative with the sum of the absolute terms that
bounds a float32 accumulation of it.

The cell of a point.  The kernels and the C oracle take pos = fma(x, scale, 0.5) in float32, floor it and subtract.  The features are
continuous in pos, but their DERIVATIVE jumps at cell faces and the fraction inherits the rounding of pos (up to 2^-13 at pos ~ 2048), so
a comparison with float32 code has to make the same rounding part of the function: fp32_cell=True rounds pos to float32 (value) and
keeps d pos / d x = scale (derivative).  fp32_cell=False is the plain float64 function, the one central differences see.

MLP part: oracle.torch_oracle.mlp_forward under autograd, with its own `half` rounding (the rounding steps x.half().float() pass the
gradient straight through; the ReLU masks are those of the rounded forward).
"""
import numpy as np
import torch

from oracle import c_oracle as co
from oracle import torch_oracle as to

PRIMES = (1, 2654435761, 805459861)
M32 = 0xFFFFFFFF


def levels(offsets, per_level_scale, base_resolution):
    """[(offset, size, scale, resolution)] per level, scale as the float32 the kernels use (gridencoder.cu:138-139)"""
    S = float(np.log2(per_level_scale))
    out = []
    for l in range(len(offsets) - 1):
        scale, res = co.level_geometry(l, S, int(base_resolution))
        out.append((int(offsets[l]), int(offsets[l + 1] - offsets[l]), float(scale), int(res)))
    return out


def grid_index(p, gridtype, size, res):
    """p [..., 3] int64 grid vertex -> entry within the level (uint32 arithmetic of gridencoder.cu:66-84, align_corners off)"""
    stride, index = 1, torch.zeros_like(p[..., 0])
    for d in range(3):
        if stride <= size:
            index = (index + p[..., d] * stride) & M32
            stride = (stride * (res + 1)) & M32
    if gridtype == 0 and stride > size:
        index = torch.zeros_like(p[..., 0])
        for d in range(3):
            index = index ^ ((p[..., d] * PRIMES[d]) & M32)
    return index % size


def _cell(x, scale, fp32_cell):
    pos = x * scale + 0.5
    if fp32_cell:
        pos = pos.detach().float().double() + (pos - pos.detach())
    pg = torch.floor(pos.detach()).long()
    return pg, pos - pg


def in_range(x):
    return ((x.detach() >= 0) & (x.detach() <= 1)).all(-1)


def grid_features(x, table, offsets, per_level_scale, base_resolution, gridtype=0, fp32_cell=True):
    """x [B, 3] float64 unit coordinates (may require grad), table [T, 2] float64 -> features [B, L, 2] float64, zero outside [0, 1]^3"""
    keep = in_range(x).double()[:, None]
    feats = []
    for off, size, scale, res in levels(offsets, per_level_scale, base_resolution):
        pg, fr = _cell(x, scale, fp32_cell)
        f = 0
        for idx in range(8):
            bits = torch.tensor([(idx >> d) & 1 for d in range(3)])
            w = torch.where(bits.bool(), fr, 1 - fr).prod(-1)
            f = f + w[:, None] * table[off + grid_index(pg + bits, gridtype, size, res)]
        feats.append(f * keep)
    return torch.stack(feats, 1)


def grid_dy_dx(x, table, offsets, per_level_scale, base_resolution, gridtype=0, fp32_cell=True):
    """the explicit derivative: d features / d x [B, L, 3, 2] float64 (the oracle's dy_dx layout), zero outside [0, 1]^3"""
    x = x.detach()
    keep = in_range(x).double()[:, None, None]
    out = []
    for off, size, scale, res in levels(offsets, per_level_scale, base_resolution):
        pg, fr = _cell(x, scale, fp32_cell)
        dy = torch.zeros(x.shape[0], 3, 2, dtype=torch.float64)
        for idx in range(8):
            bits = torch.tensor([(idx >> d) & 1 for d in range(3)])
            w = torch.where(bits.bool(), fr, 1 - fr)
            t = table[off + grid_index(pg + bits, gridtype, size, res)]
            for d in range(3):
                e0, e1 = [e for e in range(3) if e != d]
                dw = scale * (1.0 if bits[d] else -1.0) * w[:, e0] * w[:, e1]
                dy[:, d] += dw[:, None] * t
        out.append(dy * keep)
    return torch.stack(out, 1)


def grid_input_grad(x, table, offsets, per_level_scale, base_resolution, grad_enc, gridtype=0, fp32_cell=True):
    """grad_enc [L, B, 2] -> (grad_inputs [B, 3], abs_sum [B, 3]): sum over level, corner and channel of
    term = d w / d x * table[index, c] * grad_enc[level, b, c], and the sum of |term| (16 L terms per component)"""
    x = x.detach()
    keep = in_range(x).double()[:, None]
    g = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    a = torch.zeros_like(g)
    for l, (off, size, scale, res) in enumerate(levels(offsets, per_level_scale, base_resolution)):
        pg, fr = _cell(x, scale, fp32_cell)
        for idx in range(8):
            bits = torch.tensor([(idx >> d) & 1 for d in range(3)])
            w = torch.where(bits.bool(), fr, 1 - fr)
            tg = table[off + grid_index(pg + bits, gridtype, size, res)] * grad_enc[l].double()      # [B, 2]
            for d in range(3):
                e0, e1 = [e for e in range(3) if e != d]
                dw = scale * (1.0 if bits[d] else -1.0) * w[:, e0] * w[:, e1]
                g[:, d] += (dw[:, None] * tg).sum(-1)
                a[:, d] += (dw[:, None] * tg).abs().sum(-1)
    return g * keep, a * keep


# ------------------------------------------------------------------------------------------------ the MLPs
def raw_and_grad(enc, p_net, p_den, enc_dim, n_geo, half=False, dtype=torch.float64):
    """enc [P, enc_dim] -> (raw [P], d raw / d enc [P, enc_dim], margin [P], zmax): raw = MLP_den(MLP_net(enc))[0] through
    oracle.torch_oracle.mlp_forward under autograd.  margin = the sample's smallest |hidden pre-activation|, zmax the largest of all: a
    ReLU on its kink (margin ~ 0) makes the gradient discontinuous there.  half=True rounds as the oracle does (float32 arithmetic)."""
    if half:
        dtype = torch.float32
    enc = enc.detach().to(dtype).clone().requires_grad_(True)
    pn, pd = p_net.detach().to(dtype), p_den.detach().to(dtype)
    fea = to.mlp_forward(enc, pn, enc_dim, 64, 64, n_geo, 'None', half)
    raw = to.mlp_forward(fea, pd, 64, 1, 64, 1, 'None', half)[:, 0]
    (g,) = torch.autograd.grad(raw.sum(), enc)
    # the hidden pre-activations, layer by layer (the same arithmetic without the ReLU)
    with torch.no_grad():
        q = (lambda t: t.half().float()) if half else (lambda t: t)
        h = q(torch.nn.functional.pad(enc.detach(), (0, to.pad16(enc_dim) - enc_dim)))
        margin = torch.full((enc.shape[0],), float('inf'), dtype=dtype)
        zmax, off = 0.0, 0
        for o, i in to.mlp_layer_dims(enc_dim, 64, 64, n_geo)[:-1]:
            z = h @ q(pn[off:off + o * i].view(o, i)).t()
            off += o * i
            margin = torch.minimum(margin, z.abs().min(-1).values)
            zmax = max(zmax, float(z.abs().max()))
            h = q(torch.relu(z))
        fea_ = q(h @ q(pn[off:off + 64 * 64].view(64, 64)).t())
        z = fea_ @ q(pd[:64 * 64].view(64, 64)).t()
        margin = torch.minimum(margin, z.abs().min(-1).values)
        zmax = max(zmax, float(z.abs().max()))
    return raw.detach(), g.detach(), margin, zmax


def log_density_grad(ref, x, fp32_cell=True):
    """float64 autograd of log FieldRef.density at x [P, 3] (world coordinates) through the restatement: -> (grad [P, 3], margin, zmax).
    log sigma = raw + blob (trunc_exp is exp in the forward)."""
    x = x.detach().double().clone().requires_grad_(True)
    pe = ref.pos_en
    # the unit coordinates as the product computes them: in float32, (x + bound) / (2 bound); d unit / d x = 1 / (2 bound)
    unit32 = ((x.detach().float() + ref.bound) / (2 * ref.bound)).double()
    unit = unit32 + (x - x.detach()) / (2 * ref.bound)
    feats = grid_features(unit, pe.embeddings.detach().double(), pe.offsets, pe.per_level_scale, pe.base_resolution, pe.gridtype_id, fp32_cell)
    enc = feats.reshape(x.shape[0], -1)
    fea = to.mlp_forward(enc, ref.network.detach().double(), *ref.cfg_net, 'None', False)
    raw = to.mlp_forward(fea, ref.density_network.detach().double(), *ref.cfg_den, 'None', False)[:, 0]
    (g,) = torch.autograd.grad((raw + to.gaussian(x)).sum(), x)
    _, _, margin, zmax = raw_and_grad(enc, ref.network, ref.density_network, ref.enc_dim, ref.cfg_net[3])
    return g.detach(), margin, zmax


# ------------------------------------------------------------------------------------------------ the per-ray sums
def composite_normals(weights, src_index, grad_x, dirs):
    """weights [V, N, S], src_index [N, S] or None, grad_x [P, 3], dirs [N, 3] -> (normal_map [V, N, 3], orient [V, N]) in float64"""
    weights, grad_x, dirs = weights.double(), grad_x.double(), dirs.double()
    V, N, S = weights.shape
    g = grad_x[:N * S].view(N, S, 3) if src_index is None else grad_x[src_index.long()]
    q = (g * g).sum(-1, keepdim=True)
    n = torch.where(q >= 1e-20, -g / q.clamp_min(1e-300).sqrt(), torch.zeros_like(g))
    c = (n * dirs[:, None]).sum(-1).clamp_min(0)
    return (weights[..., None] * n[None]).sum(2), (weights * (c * c)[None]).sum(2)
