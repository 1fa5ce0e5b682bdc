"""docs/HISTORY.md B.27: mesh.topology and mesh.fill_holes beside mesh.remove_small_components on the marching-cubes mesh of a 512^3
sphere that the box floor cuts open; device events round the calls (host read included), two warm-ups, the median of seven alternating
repetitions; then the two passes of fill_holes alone, through the library."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from customnerf_amd import mesh  # noqa: E402
from customnerf_amd._lib import lib, check, ptr, stream  # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 512
ax = torch.linspace(-1.0, 1.0, R, device="cuda")
X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
vol = 0.8 - torch.sqrt(X ** 2 + Y ** 2 + (Z + 0.5) ** 2)                       # cut open by the volume's z = -1 face
del X, Y, Z
sp = 2.0 / (R - 1)
v, f, n = mesh.marching_cubes(vol, 0.0, spacing=(sp,) * 3, origin=(-1.0,) * 3)
del vol
V, F = v.shape[0], f.shape[0]
t = mesh.topology(v, f)
print(f"{R}^3: {V} vertices, {F} faces, {t['boundary_edges']} boundary edges in {t['boundary_loops']} loops {t['loop_lengths'].tolist()[:4]}, "
      f"euler {t['euler']}, watertight {t['watertight']}")
vo, fo, no, info = mesh.fill_holes(v, f, n)
t2 = mesh.topology(vo, fo)
print("filled:", info, "-> euler", t2['euler'], "watertight", t2['watertight'])


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ws = torch.empty(mesh.holes_workspace_bytes(V, F), dtype=torch.uint8, device="cuda")
counts = torch.empty(6, dtype=torch.int32, device="cuda")
vo, fo, no = torch.empty_like(vo), torch.empty_like(fo), torch.empty_like(no)
calls = {
    "remove_small_components": lambda: mesh.remove_small_components(v, f, n, min_faces=100),
    "topology": lambda: mesh.topology(v, f),
    "fill_holes": lambda: mesh.fill_holes(v, f, n),
    "holes_count (library)": lambda: check(lib.cnerf_mesh_holes_count(ptr(f), V, F, 0, ptr(ws), ws.numel(), ptr(counts), stream())),
    "holes_emit (library)": lambda: check(lib.cnerf_mesh_holes_emit(ptr(v), ptr(n), V, ptr(f), F, 0, ptr(ws), ws.numel(), ptr(vo), ptr(no), ptr(fo),
                                                                    vo.shape[0], fo.shape[0], stream())),
}
for _ in range(2):
    for fn in calls.values():
        fn()
times = {k: [] for k in calls}
for rep in range(7):
    for k, fn in calls.items():
        times[k].append(timed(fn))
for k, ts in times.items():
    ts = np.array(ts)
    print(f"{k}: median {np.median(ts):.3f} ms (min {ts.min():.3f}, max {ts.max():.3f})")
