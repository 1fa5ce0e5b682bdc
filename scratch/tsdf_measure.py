"""docs/HISTORY.md B.26: TSDFVolume.integrate of a 256^3 volume from 32 views of 512^2 of an analytic sphere, all views in one call
(launches of 16 views) against one call per view; device events, one warm-up, the median of seven alternating repetitions."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import tsdf_restatement as T  # noqa: E402
from customnerf_amd import mesh  # noqa: E402

R, N, S = 256, 32, 512
rng = np.random.default_rng(0)
eyes = rng.standard_normal((N, 3))
eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * 2.0
cams = np.stack([T.look_at(e) for e in eyes])
K = (880.0, 880.0, 256.0, 256.0)
depth = torch.from_numpy(np.stack([T.sphere_depth(c, 'ray', size=S, intrinsics=K) for c in cams])).cuda()
step = 1.0 / (R - 1)


def run(mode):
    tv = mesh.TSDFVolume((R, R, R), (-0.5,) * 3, (step,) * 3, 4 * step)
    tv.state                                                                     # allocated and cleared outside the timed window
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    if mode == 'single':
        for v in range(N):
            tv.integrate(depth[v], cams[v], K)
    else:
        tv.integrate(depth, cams, K)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), tv


modes = ['batched', 'single']
ref = None
for m in modes:                                                                  # warm-up, and the two forms give the same bytes
    _, tv = run(m)
    ref = tv.state.clone() if ref is None else ref
    print(m, "state equals batched:", bool(torch.equal(tv.state.view(torch.int32), ref.view(torch.int32))), "observed", tv.observed)
    del tv
times = {m: [] for m in modes}
for rep in range(7):
    for m in modes:
        times[m].append(run(m)[0])
for m in modes:
    t, launches = np.array(times[m]), N if m == 'single' else (N + 15) // 16
    byt = 16 * R ** 3 * launches
    print(f"{m}: median {np.median(t):.3f} ms (min {t.min():.3f}, max {t.max():.3f}); {launches} launches, {byt / 1e9:.3f} GB of volume traffic, "
          f"{byt / (np.median(t) * 1e-3) / 1e12:.3f} TB/s = {byt / (np.median(t) * 1e-3) / 8e12:.3f} of the 8 TB/s HBM peak")
