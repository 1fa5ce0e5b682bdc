"""Meshes that the tangent tests share (tests/test_mesh_tangent_host.py on the CPU, tests/test_gpu_mesh_tangent.py on the GPU).  A plain
module: neither test file imports the other."""
import functools

import numpy as np

import atlas_proj_restatement as AP
import atlas_proj_testlib as PL
import atlas_restatement as A
import atlas_sized_restatement as AS

f32 = np.float32


@functools.lru_cache(maxsize=None)
def hand_soup():
    """(verts, faces, uvs, normals, names): every case named.  quad: the unit square with identity UVs; mirrored: the same with u
    mirrored; det_zero: a face whose three UVs lie on a line; zero_area: a face whose three points lie on a line; seam: two faces round
    the shared vertices `seam_a` and `seam_b`, mapped into two charts that disagree there."""
    V, N, F, UV, names = [], [], [], [], {}

    def vert(p, n=(0, 0, 1)):
        V.append(p)
        N.append(n)
        return len(V) - 1

    def face(name, idx, uv):
        names[name] = len(F)
        F.append(idx)
        UV.append(uv)

    a, b, c, d = vert((0, 0, 0)), vert((1, 0, 0)), vert((1, 1, 0)), vert((0, 1, 0))
    face("quad", (a, b, c), ((0, 0), (1, 0), (1, 1)))
    face("quad_b", (a, c, d), ((0, 0), (1, 1), (0, 1)))
    a, b, c, d = vert((3, 0, 0)), vert((4, 0, 0)), vert((4, 1, 0)), vert((3, 1, 0))
    face("mirrored", (a, b, c), ((1, 0), (0, 0), (0, 1)))
    face("mirrored_b", (a, c, d), ((1, 0), (0, 1), (1, 1)))
    face("det_zero", (vert((6, 0, 0), (0.6, 0, 0.8)), vert((7, 0, 0), (0.6, 0, 0.8)), vert((6, 1, 0), (0.6, 0, 0.8))),
         ((0.25, 0.25), (0.5, 0.5), (0.75, 0.75)))
    face("zero_area", (vert((9, 0, 0), (0, 1, 0)), vert((10, 1, 1), (0, 1, 0)), vert((11, 2, 2), (0, 1, 0))), ((0, 0), (1, 0), (0, 1)))
    sa, sb = vert((12, 0, 0)), vert((12, 1, 0))
    face("seam_left", (sa, sb, vert((11.5, 0.5, 0.2))), ((0.25, 0.0), (0.25, 0.5), (0.0, 0.25)))
    face("seam_right", (sb, sa, vert((12.5, 0.5, 0.2))), ((0.75, 0.5), (0.75, 0.0), (1.0, 0.25)))
    names["seam_a"], names["seam_b"] = sa, sb
    return np.array(V, f32), np.array(F, np.int32), np.array(UV, f32), np.array(N, f32), names


def layout_uvs(layout, v, f, R, normals=None):
    """(uvs [F, 3, 2] float32, the layout's plan or None) from the layouts' own restatements"""
    if layout == 'uniform':
        return A.uvs(len(f), R), None
    if layout == 'area':
        p = AS.plan(v, f, R)
        return AS.uvs(p), p
    p = AP.plan(v, f, R, normals, g=2)
    return p.uvs.astype(f32).reshape(len(f), 3, 2), p


decimated_sphere = PL.decimated_sphere
