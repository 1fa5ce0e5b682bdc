"""GPU: the staged mesh export (customnerf_amd/nerf/mesh_export.py) where its stages share the most: a TSDF surface, smoothed, coloured
from the TSDF's own views projected onto the kept source surface, with the deviation report.  What each stage computes has its own test
file; this one checks that the combination hands every stage what it needs."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tsdf_restatement as T  # noqa: E402
from mesh_testlib import AABB, dtype_guard, gaussian_model, host  # noqa: E402,F401

RES = IMG = 24
# the test field is hazy (tests/test_gpu_mesh_tsdf.py): 0.9 lies above the haze and below the blob
VIEWS = dict(poses=np.stack([T.look_at((0, 0, 2)), T.look_at((1.2, -1.2, -1.2))]), intrinsics=(41.0, 41.0, IMG / 2.0, IMG / 2.0), H=IMG, W=IMG,
             min_opacity=0.9)


def test_tsdf_views_source_deviation_smooth_together(dtype_guard):
    model = gaussian_model(dtype_guard, False, cuda_ray=False)
    with torch.no_grad():
        model.aabb_infer.copy_(torch.tensor(AABB))                               # rays start at the box the mesh is taken from
    m = model.extract_mesh(resolution=RES, aabb=AABB, tsdf=VIEWS, color_views='tsdf', color=True, bake_from='source', deviation=True, smooth=2)
    assert set(m) == {'verts', 'faces', 'normals', 'colors', 'volume', 'threshold', 'uvs', 'texture', 'texture_layout', 'tsdf', 'view_colors',
                      'bake_kinds', 'deviation'}
    V, F = m['verts'].shape[0], m['faces'].shape[0]
    assert V > 100 and F > 100 and m['threshold'] == 0.0 and tuple(m['volume'].shape) == (RES,) * 3
    assert m['uvs'] is None and m['texture'] is None and m['texture_layout'] == 'uniform'
    assert tuple(m['colors'].shape) == (V, 3) and m['colors'].dtype == torch.uint8 and tuple(m['normals'].shape) == (V, 3)
    assert m['tsdf']['views'] == 2 and m['view_colors']['views'] == 2
    # every vertex was projected onto the kept surface once and asked of the views once: both tallies add up to V
    assert int(m['bake_kinds'].sum()) == V and int(m['view_colors']['seen'].sum()) == V and int(m['view_colors']['seen'][1:].sum()) > 0
    # smooth=2 is a lossy pass: the report is there, against the kept surface, which the smoothing has left
    assert m['deviation'] is not None and np.allclose(m['deviation']['step'], (1.0 / (RES - 1),) * 3)
    assert np.isfinite(m['deviation']['hausdorff']) and m['deviation']['hausdorff'] > 0.0
