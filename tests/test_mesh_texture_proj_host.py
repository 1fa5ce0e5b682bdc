"""CPU: the chart-based texture atlas (cnerf_mesh_atlas_proj_*).  The library's host packer against the NumPy restatement
(tests/atlas_proj_restatement.py), bit for bit, and the invariants of the restatement that the GPU tests then rely on: charts partition the
faces, rectangles are disjoint, every charted face keeps a positive UV area and at least half its area, nothing bleeds across charts under
bilinear filtering."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_proj_restatement as P  # noqa: E402
import atlas_proj_testlib as T  # noqa: E402

f32 = np.float32
EINVAL = -1


def soup():
    v, f, n, _ = T.hand_soup()
    return v, f, n


def empty():
    v, f, n, _ = T.hand_soup()
    return v, f[:0], n


# name, mesh, resolution, gutters
MESHES = [("hand_soup", soup, 64, (0, 2, 8)), ("cube", T.cube, 64, (2,)), ("quad", T.quad, 512, (0, 2, 8)),
          ("quad_at_threshold", T.quad, 36, (2,)), ("quad_over_threshold", T.quad, 37, (2,)),       # boxes of 32^2 = 1024 and 33^2 texels
          ("sphere", T.sphere_mesh, 512, (2,)),
          ("decimated_sphere", T.decimated_sphere, 256, (0, 2)), ("torus", T.torus_mesh, 1024, (2,)), ("empty", empty, 32, (2,))]
CASES = [pytest.param(get, R, g, id=f"{name}-g{g}") for name, get, R, gs in MESHES for g in gs]
_PLANS = {}


def plan_of(get, R, g):
    key = (get, R, g)
    if key not in _PLANS:
        v, f, n = get()
        _PLANS[key] = P.plan(v, f, R, n, g)
    return _PLANS[key]


def lib_pack(ext, R, g):
    """-> (status, rho, rects) of the library's packer"""
    from customnerf_amd._lib import lib
    e = np.ascontiguousarray(ext, f32).reshape(-1, 4)
    rho = C.c_double(-1.0)
    rects = np.full((len(e), 4), -9, np.int32)
    rc = lib.cnerf_mesh_atlas_proj_pack(e.ctypes.data_as(C.c_void_p), len(e), R, g, C.byref(rho), rects.ctypes.data_as(C.c_void_p))
    return rc, rho.value, rects


def same_pack(ext, R, g):
    rc, rho, rects = lib_pack(ext, R, g)
    want_rho, want = P.pack(ext, R, g)
    assert rc == 0
    assert struct.pack("<d", rho) == struct.pack("<d", want_rho), (rho, want_rho)
    np.testing.assert_array_equal(rects, want)
    return rho, rects


@pytest.mark.parametrize("get,R,g", CASES)
def test_packer_matches_restatement_on_meshes(get, R, g):
    p = plan_of(get, R, g)
    rho, rects = same_pack(p.extents, R, g)
    assert rho == p.rho


# five charts (a1 - a0, b1 - b0) at R = 24, gutter 0: the packing fits at the first and third density and not at the second
NON_MONOTONE = np.array([[0, 1.0, 0, 3.25], [0, 4.625, 0, 3.0], [0, 4.25, 0, 2.25], [0, 0.75, 0, 3.75], [0, 4.375, 0, 4.75]], f32)
NON_MONOTONE_RHO = (2.017543859649123, 2.118421052631579, 2.219298245614035)


def test_packer_hand_sets():
    one = np.array([[-1.5, 2.5, 0.25, 1.25]], f32)
    for R, g in ((16, 0), (64, 2), (100, 8), (16384, 1)):
        rho, rects = same_pack(one, R, g)
        assert rho == (R - 1 - 2 * g) / 4.0 and rects[0, 2] == R                       # the longer side spans the image
    equal = np.tile(np.array([[0, 1, 0, 0.5]], f32), (12, 1))
    rho, rects = same_pack(equal, 128, 2)
    assert len({tuple(r[2:]) for r in rects}) == 1 and rho > 0
    assert [P.shelves(NON_MONOTONE, r, 24, 0) is not None for r in NON_MONOTONE_RHO] == [True, False, True]
    rho, _ = same_pack(NON_MONOTONE, 24, 0)
    assert 0 < rho < 23 / 4.75 and P.shelves(NON_MONOTONE, rho, 24, 0) is not None     # the bisection ran and ended on a density that fits
    same_pack(np.zeros((3, 4), f32), 16, 0)                                            # charts without extent: rho = 0
    assert lib_pack(np.zeros((0, 4), f32), 16, 0)[:2] == (0, 0.0)
    # too many charts for R = 16: 5 x 5 cells of 3 x 3 texels hold 25
    many = np.tile(np.array([[0, 1, 0, 1]], f32), (26, 1))
    assert lib_pack(many, 16, 1)[0] == EINVAL
    with pytest.raises(ValueError):
        P.pack(many, 16, 1)
    same_pack(many[:25], 16, 1)
    for R, g in ((8, 0), (16385, 0), (64, 9)):
        assert lib_pack(one, R, g)[0] == EINVAL
    assert lib_pack(np.array([[1, 0, 0, 1]], f32), 64, 0)[0] == EINVAL                  # a1 < a0
    assert lib_pack(np.array([[0, np.inf, 0, 1]], f32), 64, 0)[0] == EINVAL


def test_hand_soup_is_the_mesh_it_should_be():
    v, f, n, names = T.hand_soup()
    cls = P.classes(v, f, n)
    own = P.classes(v, f, None)
    for k in ("zero_area", "repeated_index", "nan"):
        assert cls[names[k]] == 6
    assert cls[names["axis_tie"]] == 0
    assert own[names["guide_adopted"]] == 4 and cls[names["guide_adopted"]] == 0
    for k in ("guide_refused", "guide_opposite"):
        assert own[names[k]] == 4 and cls[names[k]] == 4
    assert (cls[names["minus_x"]], cls[names["minus_y"]], cls[names["sliver"]]) == (1, 3, 5)
    p = plan_of(soup, 64, 2)
    fc = p.face_chart
    assert p.C == 6 and (fc[cls == 6] == -1).all()
    assert fc[names["share_vertex_a"]] == fc[names["share_vertex_b"]]
    assert fc[names["share_nothing"]] != fc[names["share_vertex_a"]] and cls[names["share_nothing"]] == cls[names["share_vertex_a"]]
    assert fc[names["two_classes_z"]] != fc[names["two_classes_x"]]
    assert len(set(f[names["two_classes_z"]]) & set(f[names["two_classes_x"]])) == 2
    assert len(set(f[names["stacked_low"]]) & set(f[names["stacked_high"]])) == 1
    assert p.overlap > 0                                                               # the stacked pair folds over itself
    assert (p.owner_a == names["sliver"]).sum() == 0 and (p.owner_ab == names["sliver"]).sum() > 0      # pass B alone gives it texels
    assert plan_of(T.cube, 64, 2).C == 6 and plan_of(T.cube, 64, 2).overlap == 0
    q = plan_of(T.quad, 512, 2)
    assert q.C == 1 and np.bincount(q.owner_a[q.owner_a >= 0]).min() > 100_000         # faces for the cooperative path


@pytest.mark.parametrize("get,R,g", CASES)
def test_invariants(get, R, g):
    v, f, n = get()
    p = plan_of(get, R, g)
    T.check_invariants(p, v, f, R, g)
