"""profiles/mesh_view_colors.md: mesh.ViewColors on a realistic bake — the texels of a 2048^2 uniform atlas of a sphere of 8192 faces, in atlas
order, coloured from 16 views of 800^2 (analytic images, depth from mesh.rasterize, opacity weights).  Device events round accumulate
(one launch of 16 views) and resolve, one warm-up, the median of --reps repetitions; under `rocprofv3 --kernel-trace --stats` the same
launches give the kernel times.  Prints the share of texel-views that pass the depth test and the bytes the rule asks for per texel-view."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import view_colors_restatement as V  # noqa: E402
from mesh_testlib import octahedron_sphere  # noqa: E402
from customnerf_amd import mesh  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--texture", type=int, default=2048)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--views", type=int, default=16)
a = ap.parse_args()

unit, faces = octahedron_sphere(5)
v, f, n = torch.from_numpy((unit * V.RADIUS).astype(np.float32)).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(unit).cuda()
S, N = a.size, a.views
K = (1375.0 * S / 800, 1375.0 * S / 800, S / 2.0, S / 2.0)                       # the sphere fills 0.52 of the image's height from distance 2
rng = np.random.default_rng(0)
eyes = rng.standard_normal((N, 3))
eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * 2.0
cams = np.stack([V.look_at(e) for e in eyes])
rendered = [V.sphere_render(c, S, S, K) for c in cams]
images = torch.from_numpy(np.stack([r[0] for r in rendered])).cuda()
weights = torch.from_numpy(np.stack([np.isfinite(r[1]).astype(np.float32) for r in rendered])).cuda()
depth = torch.stack([mesh.rasterize(v, f, c, K, S, S)['depth'] for c in cams])
vc = mesh.ViewColors(images, depth, cams, K, 0.01, weights=weights)

got = []
mesh.bake_texture(v, f, a.texture, lambda x, d: (got.append((x.clone(), d.clone())), torch.zeros_like(x))[1], normals=n, chunk=2 ** 24)
x, d = torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])
M = x.shape[0]
nrm = (-d).contiguous()
print(f"{M} texels of a {a.texture}^2 atlas ({f.shape[0]} faces), {N} views of {S}^2")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


acc, res = [], []
for rep in range(a.reps + 1):
    state = torch.zeros(M, 4, device='cuda')
    seen = torch.zeros(M, dtype=torch.int32, device='cuda')
    t, _ = timed(lambda: vc.accumulate(x, nrm, state, seen))
    t2, out = timed(lambda: vc.resolve(state, seen))
    if rep:
        acc.append(t)
        res.append(t2)
pairs = int(seen.sum().item())
counts = (vc.counts // (a.reps + 1)).tolist()
share = pairs / (M * N)
asked = 16 + share * (48 + 16) + (16 + 4 + 16 + 4 + 24) / N                      # depths; colour + weight where seen; state, count, point, normal
acc, res = np.array(acc), np.array(res)
print(f"accumulate: median {np.median(acc):.3f} ms (min {acc.min():.3f}, max {acc.max():.3f}); resolve: median {np.median(res):.3f} ms")
print(f"texel-views that add: {pairs} of {M * N} = {share:.3f}; texels seen by 0 / 1 / >= 2 views: {counts}")
print(f"bytes asked for per texel-view: {asked:.1f} -> {asked * M * N / 1e9:.3f} GB per launch, "
      f"{asked * M * N / (np.median(acc) * 1e-3) / 1e12:.3f} TB/s of requested bytes; unique view data {(images.numel() + depth.numel() + weights.numel()) * 4 / 1e6:.0f} MB")
print(f"{np.median(acc) * 1e9 / (M * N):.2f} ps per texel-view")
