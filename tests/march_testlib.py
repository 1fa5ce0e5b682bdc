"""What the ray-march shape tests share (tests/test_gpu_raymarching_shapes.py, tests/test_oracle_independent.py): march scenes away from the
one 128^3, bound-2 sphere of the other tests, a hand-made compositing table whose interesting samples sit on the 64-sample chunk boundary
of the wave kernels, and a float64 restatement of the serial compositing loops.  A plain module: NumPy and the C oracle only, no fixtures."""
import functools
import math

import numpy as np

from oracle import c_oracle as co

F32 = np.float32

CONFIGS = ((1.0, 32), (1.5, 64), (4.0, 64), (16.0, 32))                   # (bound, H): cascades 1, 2, 3 and 5; 1.5 is no power of two
SETTINGS = ((0.0, 1024), (1.0 / 128, 1024), (1.0 / 32, 256), (0.0, 70))   # (dt_gamma, max_steps)
CAPPED = (((4.0, 64), (0.0, 1024)), ((4.0, 64), (0.0, 70)), ((16.0, 32), (0.0, 1024)), ((16.0, 32), (0.0, 70)))   # the step cap is reached
N_RAYS = 997                                                               # prime: ragged for blocks of 4 waves, for 64 and for 256


def cascades(bound):
    return 1 if bound <= 1 else 1 + int(math.ceil(math.log2(bound)))


@functools.lru_cache(maxsize=None)
def march_case(bound, H, N=N_RAYS, seed=0):
    """A raw random bitfield (30 % of the C * H^3 cells, so hits and skips alternate at every cascade) and N rays that are not a camera's:
    origins in +-1.5 bound aimed at targets in +-0.5 bound, every 5th origin pulled inside the box, directions with +0 / -0 components
    and axis-parallel ones.  -> dict(C, bitfield, o, d, aabb, nears, fars, noises); treat the arrays as read-only (the dict is cached)."""
    rng = np.random.default_rng(seed)
    C = cascades(bound)
    bitfield = np.packbits(rng.random(C * H ** 3) < 0.3, bitorder="little")
    o = ((rng.random((N, 3)) * 2 - 1) * 1.5 * bound).astype(F32)
    target = ((rng.random((N, 3)) * 2 - 1) * 0.5 * bound).astype(F32)
    noises = rng.random(N).astype(F32)
    o[::5] *= F32(0.2)                                                     # these rays start inside the box
    d = (target - o).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::13, 0] = 0.0                                                       # 1 / d = +inf in the voxel-exit distances
    d[::17, 1] = -0.0                                                      # ... and -inf, with copysign(1, -0.0) = -1
    d[::29, :2] = 0.0                                                      # parallel to the z axis
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F32)
    aabb = np.array([-bound] * 3 + [bound] * 3, F32)
    nears, fars = co.near_far_from_aabb(o, d, aabb, 0.05)
    for a in (bitfield, o, d, aabb, nears, fars, noises):
        a.setflags(write=False)
    return dict(C=C, bitfield=bitfield, o=o, d=d, aabb=aabb, nears=nears, fars=fars, noises=noises)


@functools.lru_cache(maxsize=None)
def march_oracle(bound, H, dt_gamma, max_steps, N=N_RAYS, seed=0):
    """the C oracle's exact-size march of the first N rays of march_case(bound, H): (xyzs, dirs, deltas, rays), align 128; read-only"""
    c = march_case(bound, H, N_RAYS, seed)
    out = co.march_rays_train(c["o"][:N], c["d"][:N], bound, c["bitfield"], c["C"], H, c["nears"][:N], c["fars"][:N], None, -1, c["noises"][:N], 128,
                              True, dt_gamma, max_steps)
    for a in out:
        a.setflags(write=False)
    return out


def sample_levels(xyzs, C):
    """cascade level of every sample position, as mip_from_pos derives it (raymarching.cu:42-47)"""
    mx = np.abs(xyzs).max(axis=1)
    return np.clip(np.frexp(mx)[1], 0, C - 1)


# ------------------------------------------------------------------------------------------------ compositing
TABLE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300, 64, 65, 66, 200)
TABLE_OPAQUE = {10: 62, 11: 63, 12: 64}                                   # ray -> position of its one opaque sample
TABLE_T_THRESH = 1e-4


@functools.lru_cache(maxsize=None)
def composite_table(seed=0):
    """14 rays laid out contiguously, lengths around the 64-sample chunk of the wave kernels; rays[:, 0] (the output slot) is a random
    permutation, not the identity.  Rays 10-12: sigma 0.5 and one opaque sample (sigma * dt = -ln 1e-6) at position 62 / 63 / 64, so the
    transmittance falls below T_thresh = 1e-4 just before, at and just after the chunk boundary.  Ray 13: sigma 0 but for one sample of
    1e6 (alpha == 1, T == 0 exactly).  -> dict(sigmas [M], rgbs [M, 4], deltas [M, 2], rays [14, 3], grad_ws [14], grad_image [14, 3])."""
    rng = np.random.default_rng(seed)
    lengths = np.array(TABLE_LENGTHS, np.int32)
    N, M = lengths.shape[0], int(lengths.sum())
    rays = np.zeros((N, 3), np.int32)
    rays[:, 0] = rng.permutation(N)
    assert not np.array_equal(rays[:, 0], np.arange(N))
    rays[:, 1] = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    rays[:, 2] = lengths
    dt = (0.004 + 0.004 * rng.random(M)).astype(F32)
    deltas = np.stack([dt, (dt * (1 + rng.random(M))).astype(F32)], axis=1)
    sigmas = ((3 * rng.random(M)) ** 2).astype(F32)
    rgbs = rng.random((M, 4)).astype(F32)
    for n, pos in TABLE_OPAQUE.items():
        off = rays[n, 1]
        sigmas[off:off + lengths[n]] = 0.5
        sigmas[off + pos] = F32(-np.log(1e-6) / np.float64(dt[off + pos]))
    off = rays[13, 1]
    sigmas[off:off + lengths[13]] = 0.0
    sigmas[off + 100] = 1e6
    out = dict(sigmas=sigmas, rgbs=rgbs, deltas=deltas, rays=rays, grad_ws=rng.standard_normal(N).astype(F32),
               grad_image=rng.standard_normal((N, 3)).astype(F32))
    for a in out.values():
        a.setflags(write=False)
    return out


def composite_train_f64(sigmas, rgbs, deltas, rays, T_thresh, grad_ws=None, grad_image=None):
    """The serial loops of kernel_composite_rays_train_forward / _backward (raymarching.cu:500-577, 691-772) in float64, sample by sample.
    M = len(sigmas) is the sample budget: a ray without samples or whose segment ends beyond it gives zeros and no gradient.  rgbs [M, >= 3].
    -> dict(ws, depth, image indexed by output slot; grad_sigmas [M], grad_rgbs [M, 3] (zeros without the grads); kept [M] bool: the samples
    the loop visits; margin: the smallest |ln(T / T_thresh)| at any `if (T < T_thresh) break` — how far the nearest keep decision is from
    flipping)."""
    sig, rgb, dl = np.asarray(sigmas, np.float64), np.asarray(rgbs, np.float64)[:, :3], np.asarray(deltas, np.float64)
    M, N = sig.shape[0], rays.shape[0]
    ws, depth, image = np.zeros(N), np.zeros(N), np.zeros((N, 3))
    gs, gc, kept = np.zeros(M), np.zeros((M, 3)), np.zeros(M, bool)
    margin = np.inf
    for n in range(N):
        index, offset, num_steps = (int(v) for v in rays[n])
        if num_steps == 0 or offset + num_steps > M:
            continue
        T, acc, w_sum, t, d = 1.0, np.zeros(3), 0.0, 0.0, 0.0
        for m in range(offset, offset + num_steps):                       # forward, raymarching.cu:537-566
            alpha = 1.0 - np.exp(-sig[m] * dl[m, 0])
            weight = alpha * T
            acc = acc + weight * rgb[m]
            t += dl[m, 1]
            d += weight * t
            w_sum += weight
            T *= 1.0 - alpha
            kept[m] = True
            margin = min(margin, abs(np.log(T / T_thresh)) if T > 0 else np.inf)
            if T < T_thresh:
                break
        ws[index], depth[index], image[index] = w_sum, d, acc
        if grad_ws is None:
            continue
        gw, gi = float(grad_ws[index]), np.asarray(grad_image[index], np.float64)
        T, run, w_run = 1.0, np.zeros(3), 0.0
        for m in range(offset, offset + num_steps):                       # backward, raymarching.cu:730-769
            alpha = 1.0 - np.exp(-sig[m] * dl[m, 0])
            weight = alpha * T
            run = run + weight * rgb[m]
            w_run += weight
            T *= 1.0 - alpha
            gc[m] = gi * weight
            gs[m] = dl[m, 0] * (float(np.dot(gi, T * rgb[m] - (acc - run))) + gw * (1.0 - w_sum))
            if T < T_thresh:
                break
    return dict(ws=ws, depth=depth, image=image, grad_sigmas=gs, grad_rgbs=gc, kept=kept, margin=margin)
