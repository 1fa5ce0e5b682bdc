"""Meshes that the chart-based atlas tests share (tests/test_mesh_texture_proj_host.py on the CPU, tests/test_gpu_mesh_texture_proj.py on
the GPU).  A plain module: neither test file imports the other."""
import functools
import os

import numpy as np

import atlas_proj_restatement as P

from atlas_sized_testlib import bilinear_footprint, sphere_mesh, torus_mesh, triangle_samples  # noqa: F401

f32 = np.float32


@functools.lru_cache(maxsize=None)
def hand_soup():
    """(verts, faces, normals, names): 17 faces, every case named.  Six charts: the +z faces round the hub vertex 0 (they share only that
    vertex), one +z face on its own, the +x faces round vertex `hub_x`, and one face each for -x, -y and -z (the sliver)."""
    V, N, F, names = [], [], [], {}

    def vert(p, n=(0, 0, 0)):
        V.append(p)
        N.append(n)
        return len(V) - 1

    def face(name, a, b, c):
        names[name] = len(F)
        F.append((a, b, c))

    hub = vert((0, 0, 0))
    gx, gm = (1, 0, 0), (-1, 0, 0)
    # +z faces round the hub, each in its own sector of the xy plane
    face("guide_refused", hub, vert((1, 0.1, -0.314), gx), vert((0.8, 0.7, -0.2512), gx))          # n ~ (0.3, 0, 0.95): 4 cx^2 < q
    face("guide_opposite", hub, vert((0.3, 1, -0.225), gm), vert((-0.3, 1, 0.225), gm))             # n ~ (0.6, 0, 0.8), guide -x
    face("share_vertex_a", hub, vert((-0.5, 1, 0)), vert((-1, 0.6, 0)))
    face("share_vertex_b", hub, vert((-1, 0.3, 0)), vert((-1, -0.3, 0)))
    face("stacked_low", hub, vert((-1, -0.5, 0)), vert((-0.3, -1, 0)))
    face("stacked_high", hub, vert((-1, -0.5, 1)), vert((-0.3, -1, 1)))                             # the same projection, one vertex shared
    a, b = vert((1, -1, 0)), vert((1, -0.2, 0))
    face("two_classes_z", hub, a, b)
    hub_x = vert((1, -0.6, -1))
    face("two_classes_x", b, a, hub_x)                                                              # across the edge a-b: +x
    face("axis_tie", hub_x, vert((1, -0.6, 0)), vert((2, -1.6, -1)))                                # c = (1, 1, 0): the lowest axis
    face("guide_adopted", hub_x, vert((2, -0.4, -1.75), gx), vert((1.5, 0.4, -1.375), gx))          # n ~ (0.6, 0, 0.8), guide +x
    face("share_nothing", vert((2, 2, 0)), vert((3, 2, 0)), vert((2, 3, 0)))                        # +z, a chart of its own
    face("minus_x", vert((0, 0, 0)), vert((0, 0, 1)), vert((0, 1, 0)))
    face("minus_y", vert((0, 0, 0)), vert((1, 0, 0)), vert((0, 0, 1)))
    face("sliver", vert((0, 0.1, 0)), vert((1, 0.00013, 0)), vert((0.99, 0.00003, 0)))              # -z, thinner than a texel
    face("zero_area", vert((0, 0, 0)), vert((1, 1, 1)), vert((2, 2, 2)))
    r = vert((0.5, 0.5, 0.5))
    face("repeated_index", r, r, vert((1, 0, 0)))
    face("nan", vert((0, 0, 0)), vert((float("nan"), 0, 0)), vert((0, 1, 0)))
    names["hub_x"] = hub_x
    return np.array(V, f32), np.array(F, np.int32), np.array(N, f32), names


@functools.lru_cache(maxsize=None)
def cube():
    """12 faces wound outwards on 8 vertices"""
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], f32)      # index 4 x + 2 y + z
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # -x, +x, -y, +y, -z, +z
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int32), None


@functools.lru_cache(maxsize=None)
def quad():
    """two faces: at 512 texels each covers more than 10^5"""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], f32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), None


@functools.lru_cache(maxsize=None)
def decimated_sphere():
    """(verts, faces, normals) of sphere_mesh() decimated to 300 faces by mesh.decimate(v, f, 300, normals=n): large irregular faces with
    decimated normals, the shape save_mesh(target_faces=) produces.  Stored (tests/golden/atlas_proj_decimated_sphere.npz) so that the
    CPU tests have it; tests/test_gpu_mesh_texture_proj.py checks that the decimation still gives these arrays."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atlas_proj_decimated_sphere.npz"))
    return z["verts"], z["faces"], z["normals"]


def check_invariants(p, v, f, R, g):
    """what must hold of a plan p (atlas_proj_restatement.plan) of the mesh (v, f) whatever the mesh: charts partition the charted faces,
    rectangles are disjoint and inside the image, every charted face has a positive UV area and keeps half its area in projection, owned
    texels lie inside their chart's rectangle (inside the gutter before growth), and for g >= 1 a bilinear lookup inside a charted face
    reads texels of its chart only"""
    cls, fc = p.classes, p.face_chart
    charted = fc >= 0
    # charts partition the charted faces; one class per chart; faces sharing a vertex in one class share the chart
    assert ((cls < 6) == charted).all() and sorted(set(fc[charted])) == list(range(p.C))
    for c in range(p.C):
        assert len(set(cls[fc == c])) == 1
    seen = {}
    for i in np.nonzero(charted)[0]:
        for q in f[i]:
            assert seen.setdefault((int(q), int(cls[i])), fc[i]) == fc[i]
    # rectangles are disjoint and inside the image
    rc = p.rects
    assert (rc[:, :2] >= 0).all() and (rc[:, 0] + rc[:, 2] <= R).all() and (rc[:, 1] + rc[:, 3] <= R).all()
    paint = np.zeros((R, R), np.int32)
    for x, y, w, h in rc:
        paint[y:y + h, x:x + w] += 1
    assert paint.max(initial=0) <= 1
    if not charted.any():
        assert p.total == 0
        return
    # positive UV area, and at least half the area survives the projection
    uv = p.uvs.astype(np.float64)[charted]
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()
    a, b = P.project(v, f, cls)
    a, b = a.astype(np.float64)[charted], b.astype(np.float64)[charted]
    proj = 0.5 * ((a[:, 1] - a[:, 0]) * (b[:, 2] - b[:, 0]) - (b[:, 1] - b[:, 0]) * (a[:, 2] - a[:, 0]))
    tri = v[f[charted]].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (2 * proj >= area * (1 - 1e-5)).all(), (2 * proj / area).min()             # float32 classification: |n . axis| >= 0.5 to 2^-20 or so
    # owned texels lie in the owner's chart's rectangle, inside the gutter before growth
    for own, inset in ((p.owner_ab, g), (p.owner, 0)):
        Y, X = np.nonzero(own >= 0)
        r = rc[fc[own[Y, X]]]
        assert (X >= r[:, 0] + inset).all() and (X < r[:, 0] + r[:, 2] - inset).all()
        assert (Y >= r[:, 1] + inset).all() and (Y < r[:, 1] + r[:, 3] - inset).all()
    # the seam invariant: every texel under a bilinear lookup inside a charted face belongs to its chart
    if g >= 1:
        rng = np.random.default_rng(5)
        chart_map = np.where(p.owner >= 0, fc[np.maximum(p.owner, 0)], -1)
        faces = np.nonzero(charted)[0]
        if len(faces) > 1500:
            faces = faces[rng.permutation(len(faces))[:1500]]
        for i in faces:
            pts = triangle_samples(np.stack([p.tx[i], p.ty[i]], -1) - 0.5, rng, k_edge=5, k_in=12)
            X, Y = bilinear_footprint(pts)
            assert (chart_map[Y, X] == fc[i]).all(), i
