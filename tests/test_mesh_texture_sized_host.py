"""CPU: the area-proportional texture atlas of csrc/mesh_texture.hip through its NumPy restatement (tests/atlas_sized_restatement.py) and the
library's host-only layout function (cnerf_mesh_atlas_sized_layout): the threshold e is the smallest that fits, the capacity edge, argument
checks, the geometry of the plan (disjoint aligned cells, the fill predicate, the seam invariant), the density bound that follows from the
rules, and the size keys at their edges.  No GPU compute is issued here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import atlas_sized_restatement as S  # noqa: E402
import atlas_sized_testlib as T  # noqa: E402


def lib_layout(hist, R):
    """cnerf_mesh_atlas_sized_layout -> (rc, e, counts [8], tiles)"""
    from customnerf_amd._lib import lib
    h = (C.c_uint32 * 2048)(*[int(x) for x in hist])
    e, tiles, counts = C.c_uint32(77), C.c_uint32(77), (C.c_uint32 * 8)()
    rc = lib.cnerf_mesh_atlas_sized_layout(h, int(R), C.byref(e), counts, C.byref(tiles))
    return rc, e.value, np.array(list(counts), np.int64), tiles.value


def mesh_histograms():
    v, f, _, _ = T.hand_soup()
    yield "hand_soup", S.histogram(S.size_keys(v, f)[0]), (64, 128, 16384)
    v, f = T.random_soup()
    yield "random_soup", S.histogram(S.size_keys(v, f)[0]), (256, 512, 1024)
    v, f, _ = T.sphere_mesh()
    yield "sphere", S.histogram(S.size_keys(v, f)[0]), (256, 512)
    v, f, _ = T.torus_mesh()
    yield "torus", S.histogram(S.size_keys(v, f)[0]), (2048,)


def random_histograms():
    rng = np.random.default_rng(11)
    for i in range(24):
        h = np.zeros(2048, np.int64)
        centre, width, F = rng.integers(100, 1900), rng.integers(1, 120), int(rng.integers(1, 40_000))
        keys = np.clip(np.rint(rng.normal(centre, width, F)), 0, 2047).astype(np.int64)
        np.add.at(h, keys, 1)
        yield f"random{i}", h, (int(2 ** rng.integers(4, 15)),)


def test_e_is_the_smallest_that_fits():
    """tiles(e) <= (R / 4)^2 < tiles(e - 1) whenever e > 0, and the library's e, counts and tiles are the restatement's"""
    seen_e = set()
    for name, h, Rs in list(mesh_histograms()) + list(random_histograms()):
        for R in Rs:
            K, cap = S.classes_of(R), (R // 4) ** 2
            rc, e, n, tiles = lib_layout(h, R)
            if (int(h.sum()) + 1) // 2 > cap:
                assert rc == -1, (name, R)
                with pytest.raises(ValueError):
                    S.layout(h, R)
                continue
            assert rc == 0, (name, R)
            er, nr, tr = S.layout(h, R)
            assert (e, tiles) == (er, tr) and np.array_equal(n, nr), (name, R)
            assert n.sum() == h.sum() and (n[K + 1:] == 0).all()
            assert S.tiles_of(S.class_counts(h, e, K)) == tiles <= cap
            if e > 0:
                assert S.tiles_of(S.class_counts(h, e - 1, K)) > cap, (name, R)
            seen_e.add(e > 0)
    assert seen_e == {False, True}                                             # both an atlas with room to spare and a tight one were seen


def test_tiles_is_not_monotone_so_e_is_found_by_scanning():
    """two faces one key apart: moving one of them down a class opens a cell there without closing one above, so tiles(e) rises"""
    h = np.zeros(2048, np.int64)
    h[[100, 101]] = 1
    t = [S.tiles_of(S.class_counts(h, e, 4)) for e in (84, 85, 86)]
    assert t == [4, 5, 1]
    h[1500] = 9                                                               # cap 16 tiles at R = 16: 5 cells of class 0 and ... no class 2
    rc, e, n, tiles = lib_layout(h, 16)
    assert rc == 0 and (e, tiles) == S.layout(h, 16)[::2]


def test_capacity_edge():
    h = np.zeros(2048, np.int64)
    h[1000] = 32
    rc, e, n, tiles = lib_layout(h, 16)
    assert rc == 0 and tiles == 16 and list(n) == [32, 0, 0, 0, 0, 0, 0, 0]
    h[1000] = 33
    assert lib_layout(h, 16)[0] == -1
    h[:] = 0
    h[[3, 500, 2047]] = (10, 11, 12)                                           # spread over every class: still 33 faces
    assert lib_layout(h, 16)[0] == -1
    h[3] = 9
    rc, e, n, tiles = lib_layout(h, 16)
    assert rc == 0 and tiles == 16 and list(n)[:3] == [32, 0, 0]
    rc, e, n, tiles = lib_layout(np.zeros(2048, np.int64), 16)                 # F = 0: e = 0 and no cell
    assert (rc, e, tiles) == (0, 0, 0) and not n.any()


def test_argument_checks():
    from customnerf_amd._lib import lib
    from customnerf_amd import mesh
    h = np.zeros(2048, np.int64)
    h[700] = 4
    for R in (8, 15, 17, 24, 100, 1000, 16383, 16385, 32768, 0):
        assert lib_layout(h, R)[0] == -1, R
        with pytest.raises(ValueError):
            S.classes_of(R)
    for R in (16, 64, 16384):
        assert lib_layout(h, R)[0] == 0, R
    e, t, n = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 8)()
    hh = (C.c_uint32 * 2048)()
    assert lib.cnerf_mesh_atlas_sized_layout(None, 64, C.byref(e), n, C.byref(t)) == -2
    assert lib.cnerf_mesh_atlas_sized_layout(hh, 64, None, n, C.byref(t)) == -2
    nbytes = C.c_uint64(0)
    assert lib.cnerf_mesh_atlas_sized_workspace_bytes(1000, C.byref(nbytes)) == 0 and nbytes.value >= 256 + 1000 * 12
    assert lib.cnerf_mesh_atlas_sized_workspace_bytes(2 ** 25 + 1, C.byref(nbytes)) == -1
    one = C.c_void_p(16)                                                        # non-NULL dummy, never dereferenced on these paths
    n[0] = 4
    assert lib.cnerf_mesh_atlas_sized_plan(4, 48, 0, n, one, 1 << 20, one, one, 4, None) == -1          # R no power of two
    assert lib.cnerf_mesh_atlas_sized_plan(5, 64, 0, n, one, 1 << 20, one, one, 5, None) == -1          # counts are no partition of F
    assert lib.cnerf_mesh_atlas_sized_plan(4, 64, 2049, n, one, 1 << 20, one, one, 4, None) == -1       # e
    assert lib.cnerf_mesh_atlas_sized_plan(4, 64, 0, n, one, 16, one, one, 4, None) == -1               # workspace too small
    n[0], n[5] = 3, 1
    assert lib.cnerf_mesh_atlas_sized_plan(4, 64, 0, n, one, 1 << 20, one, one, 4, None) == -1          # a class above K = 4
    n[5], n[4] = 0, 1
    assert lib.cnerf_mesh_atlas_sized_plan(4, 64, 0, n, one, 1 << 20, one, one, 4, None) == -1          # 256 + 2 tiles on 256
    assert lib.cnerf_mesh_atlas_sized_points(one, None, 3, one, 4, 64, n, one, 1 << 20, 0, 16, one, one, one, 16, None) == -1
    assert lib.cnerf_mesh_atlas_sized_fill(64, 257, (C.c_uint8 * 3)(), one, None) == -1
    assert lib.cnerf_mesh_atlas_sized_fill(48, 1, (C.c_uint8 * 3)(), one, None) == -1
    import torch
    with pytest.raises(RuntimeError):                                           # no CPU path
        mesh.atlas_plan(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), 64)
    with pytest.raises(RuntimeError):
        mesh.bake_texture(torch.zeros(3, 3), torch.tensor([[0, 1, 2]]), 64, lambda x, d: x, layout='area')


PLANS = [("hand_soup", 64, None), ("hand_soup", 64, 1080), ("hand_soup", 256, None), ("random_soup", 256, None), ("sphere", 512, None)]


def _plan(name, R, e):
    v, f = {"hand_soup": T.hand_soup, "random_soup": T.random_soup, "sphere": T.sphere_mesh}[name]()[:2]
    return S.plan(v, f, R, e=e)


@pytest.mark.parametrize("name,R,e", PLANS, ids=[f"{n}_R{r}_e{e}" for n, r, e in PLANS])
def test_plan_geometry(name, R, e):
    p = _plan(name, R, e)
    c = p.cells.astype(np.int64)
    X0, Y0, s, b = c.T
    # cells: inside the image, aligned to their size, two faces at most per cell and those A and B, pairwise disjoint (owner_map asserts it)
    assert (X0 >= 0).all() and (Y0 >= 0).all() and (X0 + s <= R).all() and (Y0 + s <= R).all()
    assert (X0 % s == 0).all() and (Y0 % s == 0).all() and np.isin(s, 4 << np.arange(p.K + 1)).all()
    cell_id = (Y0 * R + X0) * 2 + b
    assert len(np.unique(cell_id)) == p.F
    own = S.owner_map(p)
    covered = np.zeros((R, R), bool)
    for x0, y0, ss in {(int(a), int(bb), int(cc)) for a, bb, cc in zip(X0, Y0, s)}:
        assert not covered[y0:y0 + ss, x0:x0 + ss].any()
        covered[y0:y0 + ss, x0:x0 + ss] = True
    # the fill predicate: a texel is in a cell iff its Morton code is below tiles
    assert np.array_equal(covered, S.in_cells(p)) and covered.sum() == p.texels == 16 * p.tiles
    assert not (own[~covered] >= 0).any()
    # the texel order visits every cell texel once, and its owners are the owner map's
    face, i, j, X, Y, st = S.cell_texels(p)
    assert len(np.unique(Y * R + X)) == p.texels and covered[Y, X].all()
    assert np.array_equal(own[Y, X], face)
    odd = [k for k in range(8) if p.n[k] % 2]
    assert (face < 0).sum() == sum((4 << k) ** 2 - (4 << k) * ((4 << k) + 1) // 2 for k in odd)
    # the seam invariant, on a dense set of points per triangle, in every class present
    rng = np.random.default_rng(R)
    XY = S.corner_texels(p).astype(np.float64)
    checked = set()
    for f in np.concatenate([rng.permutation(np.nonzero(p.k == k)[0])[:80] for k in range(8)]):      # every class present; all of a small mesh
        X, Y = T.bilinear_footprint(T.triangle_samples(XY[f], rng, k_edge=2 * int(s[f]), k_in=20 * int(s[f])))
        assert ((X >= 0) & (X < R) & (Y >= 0) & (Y < R)).all() and (own[Y, X] == f).all(), f
        checked.add(int(p.k[f]))
    assert checked == set(np.nonzero(p.n)[0].tolist())
    # UVs decode to the corner texels and wind counter-clockwise with v up
    uv = S.uvs(p).astype(np.float64)
    assert np.abs(uv[..., 0] * R - 0.5 - XY[..., 0]).max() < 1e-3 and np.abs((1 - uv[..., 1]) * R - 0.5 - XY[..., 1]).max() < 1e-3
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    assert (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0] > 0).all()


def test_hand_soup_reaches_every_branch():
    """what the GPU tests rely on: at R = 64 the soup has four classes, one with an odd count (an un-owned B), one with a single face"""
    v, f, _, names = T.hand_soup()
    p = S.plan(v, f, 64)
    present = p.n[p.n > 0]
    assert len(present) >= 4 and (present % 2 == 1).any() and (present == 1).any() and len(f) == 41


@pytest.mark.parametrize("R", [256, 512, 1024])
def test_density_bound(R):
    """For 1 <= k < K the key rule puts L2 / threshold^2 in [4^k, 4^(k + 1)), so (s - 2) / sqrt(L2) * threshold lies in
    (2 - 2^-k, 4 - 2^(1 - k)], inside (1.5, 4): texels per unit length vary by less than 8 / 3 across those classes."""
    v, f = T.random_soup()
    p = S.plan(v, f, R)
    m = (p.k >= 1) & (p.k < p.K)
    assert m.sum() > 400
    dens = ((4 << p.k[m]) - 2) / np.sqrt(p.L2[m].astype(np.float64)) * S.threshold(p.e)
    print(f"R = {R}: e = {p.e}, counts {p.n.tolist()}, density x threshold in [{dens.min():.4f}, {dens.max():.4f}]")
    assert dens.min() > 1.5 and dens.max() < 4


def test_key_edges():
    v, f, _, names = T.hand_soup()
    keys, L2 = S.size_keys(v, f)
    b, u = names["boundary"], names["below_boundary"]
    assert L2[b] == 1024.0 and keys[b] == (np.array([1024], np.float32).view(np.uint32)[0] >> 20) == 1096
    assert L2[u] < 1024.0 and keys[u] == 1095                                   # the float below 32, squared: the bin under the boundary
    assert L2[names["zero_area"]] > 0 and keys[names["zero_area"]] > 0         # collinear: it still has a longest edge
    assert L2[names["zero_length"]] == 0 and keys[names["zero_length"]] == 0
    d = L2[names["denormal"]]
    assert 0 < d < np.finfo(np.float32).tiny and keys[names["denormal"]] == 0
    assert np.isinf(L2[names["overflow"]]) and keys[names["overflow"]] == 0
    assert keys.min() >= 0 and keys.max() <= 2047
    # with the threshold 16 keys under the boundary the two faces part: class 1 and class 0
    p = S.plan(v, f, 64, e=1096 - 16)
    assert p.k[b] == 1 and p.k[u] == 0
    # the degenerate faces are class 0 at the layout's own e and own a smallest cell each
    p = S.plan(v, f, 64)
    for name in ("zero_area", "zero_length", "denormal", "overflow"):
        assert p.k[names[name]] == 0 and p.cells[names[name], 2] == 4, name
    # a NaN edge beside numbers is ignored; a face of NaNs has key 0
    vn = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan] * 3, [np.inf, 0, 0]], np.float32)
    kn, _ = S.size_keys(vn, np.array([[0, 1, 2], [3, 3, 3], [0, 1, 3], [4, 4, 0]]))
    assert kn[0] == (np.array([5], np.float32).view(np.uint32)[0] >> 20) and kn[1] == 0 and kn[2] == (np.array([4], np.float32).view(np.uint32)[0] >> 20)
    assert kn[3] == 0
    assert S.threshold(1096) == 32.0 and S.threshold(2048) == np.inf
