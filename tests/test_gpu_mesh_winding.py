"""GPU: the generalized winding number, the inside test and the signed distance on the mesh BVH (csrc/mesh_bvh.hip, k_bvh_moments_leaf /
k_bvh_moments_fit / k_bvh_winding / k_bvh_signed) against tests/winding_restatement.py over the fixtures and ~2000 queries each of
tests/winding_testlib.py: the moments buffer bit-equal to its float32 restatement; queries that write nothing but their outputs; w within
n_terms 2^-20 of the restated walk, whose accept decisions the device must share (the stats are equal); at beta = inf the same bound
against the exact float64 sum; `contains` equal to the reference outside the band; the signed distance made of closest_point's bits and
that sign; nested, inward-wound and broken meshes; two runs and two batchings identical; pruning.

The bound: a term is at most 1/2 in size and its float32 error a few units of 2^-24 (the rounding of the products, atan2f, the running
sum); 2^-20 per term leaves a factor of 16.  Measured on the device (printed by test_winding_against_the_restated_walk and
test_exact_sum_at_beta_inf): the largest |dw| / n_terms is 1.26e-8 at beta = 2 and 1.86e-8 at beta = inf, both on the
nested spheres.

ON the surface w is discontinuous — it jumps by one across a face — and the exact sum there is decided by the rounding of the query: the
comparisons with the EXACT reference (beta = inf, `contains`) are made for the queries at least 1e-6 diagonals off the surface, the
condition the reference itself is held to (tests/test_mesh_winding_host.py (a)).  The queries on the surface (vertices, centroids) take
part in everything else: against the restated walk, whose float32 decisions are the device's, nothing is exempt."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import winding_testlib as L  # noqa: E402
from mesh_testlib import cuda  # noqa: E402

SENTINEL = -7.0
PAD = 8
FILL = 0x5a
TERM = 2.0 ** -20


def _p(t):
    from customnerf_amd._lib import ptr
    return None if t is None or not t.numel() else ptr(t)


def gpu_tree(v, f):
    """cnerf_mesh_bvh_build and cnerf_mesh_winding_build into over-allocated, byte-filled buffers -> dict"""
    from customnerf_amd import mesh
    from customnerf_amd._lib import lib, check, ptr, stream
    gv, gf = cuda(np.asarray(v, np.float32)), cuda(np.asarray(f, np.int32))
    V, F = len(v), len(f)
    nbytes, mbytes = mesh.bvh_workspace_bytes(V, F), mesh.winding_workspace_bytes(V, F)
    ws = torch.full((nbytes + 256,), FILL, dtype=torch.uint8, device="cuda")
    mom = torch.full((mbytes + 256,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int32, device="cuda")
    check(lib.cnerf_mesh_bvh_build(_p(gv), V, _p(gf), F, ptr(ws), nbytes, ptr(counts), stream()), "build")
    built = ws.clone()
    check(lib.cnerf_mesh_winding_build(ptr(ws), nbytes, V, F, ptr(mom), mbytes, stream()), "winding_build")
    torch.cuda.synchronize()
    assert torch.equal(ws, built)                                                  # the moments' build reads the tree and writes none of it
    return {'ws': ws, 'nbytes': nbytes, 'mom': mom, 'mbytes': mbytes, 'V': V, 'F': F, 'n': int(counts[0])}


def gpu_winding(t, q, beta):
    """cnerf_mesh_winding_query into sentinel-padded buffers -> (w [Q] float32, stats); tree, moments and padding are checked"""
    from customnerf_amd._lib import lib, check, ptr, stream
    ws0, mom0 = t['ws'].clone(), t['mom'].clone()
    Q = len(q)
    gq = cuda(np.asarray(q, np.float32))
    w = torch.full((Q + PAD,), SENTINEL, device="cuda")
    stats = torch.zeros(2 + PAD, dtype=torch.int64, device="cuda")
    check(lib.cnerf_mesh_winding_query(ptr(t['ws']), t['nbytes'], t['V'], t['F'], ptr(t['mom']), t['mbytes'], _p(gq), Q, float(beta), ptr(w),
                                       ptr(stats), stream()), "winding_query")
    torch.cuda.synchronize()
    assert torch.equal(t['ws'], ws0) and torch.equal(t['mom'], mom0)
    w, s = w.cpu().numpy(), stats.cpu().numpy()
    assert (w[Q:] == SENTINEL).all() and (s[2:] == 0).all()
    return w[:Q], (int(s[0]), int(s[1]))


def gpu_signed(t, q, beta, want_w=True):
    from customnerf_amd._lib import lib, check, ptr, stream
    ws0, mom0 = t['ws'].clone(), t['mom'].clone()
    Q = len(q)
    gq = cuda(np.asarray(q, np.float32))
    sd = torch.full((Q + PAD,), SENTINEL, device="cuda")
    face = torch.full((Q + PAD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    w = torch.full((Q + PAD,), SENTINEL, device="cuda") if want_w else None
    stats = torch.zeros(2 + PAD, dtype=torch.int64, device="cuda")
    check(lib.cnerf_mesh_bvh_signed_distance(ptr(t['ws']), t['nbytes'], t['V'], t['F'], ptr(t['mom']), t['mbytes'], _p(gq), Q, float(beta),
                                             ptr(sd), ptr(face), _p(w), ptr(stats), stream()), "signed_distance")
    torch.cuda.synchronize()
    assert torch.equal(t['ws'], ws0) and torch.equal(t['mom'], mom0)
    out = {'signed': sd.cpu().numpy(), 'face': face.cpu().numpy(), 'stats': tuple(int(x) for x in stats.cpu().numpy()[:2])}
    assert (out['signed'][Q:] == SENTINEL).all() and (out['face'][Q:] == int(SENTINEL)).all() and (stats.cpu().numpy()[2:] == 0).all()
    out['signed'], out['face'] = out['signed'][:Q], out['face'][:Q]
    if want_w:
        a = w.cpu().numpy()
        assert (a[Q:] == SENTINEL).all()
        out['winding'] = a[:Q]
    return out


@functools.lru_cache(maxsize=None)
def run(name):
    """the device's answers for a fixture, computed once: tree, w2 / stats2 (beta = 2), winf / statsinf (beta = inf), sd (signed, beta = 2)"""
    c = L.case(name)
    t = gpu_tree(c['v'], c['f'])
    w2, s2 = gpu_winding(t, c['q'], 2.0)
    winf, sinf = gpu_winding(t, c['q'], math.inf)
    return {'tree': t, 'w2': w2, 'stats2': s2, 'winf': winf, 'statsinf': sinf, 'sd': gpu_signed(t, c['q'], 2.0)}


@pytest.mark.parametrize("name", L.NAMES)
def test_moments_bit_equal(name):
    c, t = L.case(name), run(name)['tree']
    assert t['n'] == c['tree']['n']
    want = c['mom']                                                                # [2^(D + 1), 2, 4]
    raw = t['mom'].cpu().numpy()
    got = raw[:32 * len(want)].view(np.uint32).reshape(-1, 2, 4)
    np.testing.assert_array_equal(got[1:], want[1:].view(np.uint32))
    assert (raw[:32] == FILL).all() and (raw[32 * len(want):] == FILL).all()       # index 0, deeper levels that do not exist, the padding


@pytest.mark.parametrize("name", L.NAMES)
def test_winding_against_the_restated_walk(name):
    c, r = L.case(name), run(name)
    n_terms = c['acc2'] + c['tri2']
    err = np.abs(r['w2'].astype(np.float64) - c['w2'])
    worst = float((err / np.maximum(n_terms, 1)).max())
    print(f"{name}: beta = 2, max |dw| / n_terms = {worst:.3g} (bound {TERM:.3g}), max |dw| = {float(err.max()):.3g}, stats {r['stats2']}")
    assert r['stats2'] == (int(c['acc2'].sum()), int(c['tri2'].sum()))            # the same accept decisions
    assert (err <= n_terms * TERM).all()
    fin = np.isfinite(c['q']).all(1)
    assert (r['w2'][~fin] == 0).all() and (r['winf'][~fin] == 0).all()


@pytest.mark.parametrize("name", L.NAMES)
def test_exact_sum_at_beta_inf(name):
    c, r = L.case(name), run(name)
    assert r['statsinf'] == (0, int(c['triinf'].sum()))
    off = c['off']
    err = np.abs(r['winf'].astype(np.float64) - c['exact'])[off]
    n_terms = c['triinf'][off]
    if off.any():
        print(f"{name}: beta = inf, max |w - exact| / n_terms = {float((err / np.maximum(n_terms, 1)).max()):.3g} (bound {TERM:.3g})")
    assert (err <= n_terms * TERM).all()
    # and against the restated walk, the queries on the surface included
    assert (np.abs(r['winf'].astype(np.float64) - c['winf']) <= c['triinf'] * TERM).all()


@pytest.mark.parametrize("name", L.NAMES)
def test_contains_equals_the_reference(name):
    from customnerf_amd import mesh
    c, r = L.case(name), run(name)
    ask = c['clear'] & c['off']
    want = c['exact'] >= 0.5
    for w in (r['w2'], r['winf']):
        np.testing.assert_array_equal((w >= 0.5)[ask], want[ask])
    bvh = mesh.build_bvh(cuda(c['v']), cuda(c['f']))
    assert bvh.moments is None
    q = cuda(c['q'])
    for beta, w in ((2.0, r['w2']), (math.inf, r['winf'])):
        np.testing.assert_array_equal(mesh.contains(bvh, q, beta).cpu().numpy(), w >= 0.5)
        np.testing.assert_array_equal(mesh.winding_number(bvh, q, beta).cpu().numpy().view(np.uint32), w.view(np.uint32))
    assert bvh.moments is not None                                                 # built on first use, kept
    w, stats = mesh.winding_number(bvh, q, want_stats=True)
    assert stats == r['stats2']


@pytest.mark.parametrize("name", L.NAMES)
def test_signed_distance(name):
    from customnerf_amd import mesh
    c, r = L.case(name), run(name)
    sd = r['sd']
    bvh = mesh.build_bvh(cuda(c['v']), cuda(c['f']))
    q = cuda(c['q'])
    cp = mesh.closest_point(bvh, q)
    dist = np.sqrt(cp['dist2'].cpu().numpy())                                      # float32, correctly rounded
    np.testing.assert_array_equal(np.abs(sd['signed']).view(np.uint32), dist.view(np.uint32))
    np.testing.assert_array_equal(sd['face'], cp['face'].cpu().numpy())
    np.testing.assert_array_equal(sd['winding'].view(np.uint32), r['w2'].view(np.uint32))
    fin = np.isfinite(c['q']).all(1) & (c['tree']['n'] > 0)
    np.testing.assert_array_equal(np.signbit(sd['signed']), r['w2'] >= 0.5)
    assert (sd['signed'][~fin] == np.inf).all() and (sd['face'][~fin] == -1).all() and (sd['winding'][~fin] == 0).all()
    assert sd['stats'] == r['stats2']
    out = mesh.signed_distance(bvh, q, want_winding=True, want_stats=True)
    np.testing.assert_array_equal(out['signed'].cpu().numpy().view(np.uint32), sd['signed'].view(np.uint32))
    np.testing.assert_array_equal(out['face'].cpu().numpy(), sd['face'])
    np.testing.assert_array_equal(out['winding'].cpu().numpy().view(np.uint32), sd['winding'].view(np.uint32))
    assert out['stats'] == sd['stats'] and out['signed'].dtype == torch.float32 and out['face'].dtype == torch.int32
    assert sorted(mesh.signed_distance(bvh, q)) == ['face', 'signed']
    no_w = gpu_signed(r['tree'], c['q'], 2.0, want_w=False)
    np.testing.assert_array_equal(no_w['signed'].view(np.uint32), sd['signed'].view(np.uint32))


def test_nested_and_inward():
    c, r = L.case("nested"), run("nested")
    rad = np.linalg.norm(c['q'].astype(np.float64), axis=1)
    inner, between, outside = rad < 0.45, (rad > 0.55) & (rad < 0.9), (rad > 1.05) & np.isfinite(rad)
    assert inner.sum() >= 19 and between.sum() >= 50 and outside.sum() >= 500
    for w in (r['w2'], r['winf']):
        assert (np.round(w[inner]) == 2).all() and (np.round(w[between]) == 1).all() and (np.round(w[outside]) == 0).all()
    c, r = L.case("inward"), run("inward")
    rad = np.linalg.norm(c['q'].astype(np.float64), axis=1)
    for w in (r['w2'], r['winf']):
        assert (np.round(w[rad < 0.9]) == -1).all() and (rad < 0.9).sum() >= 50 and not (w >= 0.5).any()
    assert (r['sd']['signed'] >= 0).all()                                          # nothing is inside an inward-wound mesh


@pytest.mark.parametrize("name", ["torus", "soup", "holed_sphere"])
def test_two_runs_and_two_batchings_are_identical(name):
    c, r = L.case(name), run(name)
    t, q = r['tree'], c['q']
    for beta, first in ((2.0, r['w2']), (math.inf, r['winf'])):
        again, _ = gpu_winding(t, q, beta)
        np.testing.assert_array_equal(again.view(np.uint32), first.view(np.uint32))
        cut = 1001                                                                 # not a multiple of the wave or the workgroup
        a, sa = gpu_winding(t, q[:cut], beta)
        b, sb = gpu_winding(t, q[cut:], beta)
        np.testing.assert_array_equal(np.concatenate([a, b]).view(np.uint32), first.view(np.uint32))
        assert (sa[0] + sb[0], sa[1] + sb[1]) == (r['stats2'] if beta == 2.0 else r['statsinf'])
    sd = gpu_signed(t, q, 2.0)
    np.testing.assert_array_equal(sd['signed'].view(np.uint32), r['sd']['signed'].view(np.uint32))
    a, b = gpu_signed(t, q[:cut], 2.0), gpu_signed(t, q[cut:], 2.0)
    np.testing.assert_array_equal(np.concatenate([a['signed'], b['signed']]).view(np.uint32), r['sd']['signed'].view(np.uint32))
    np.testing.assert_array_equal(np.concatenate([a['face'], b['face']]), r['sd']['face'])


def test_bad_faces_answer_as_the_mesh_without_them():
    good, bad = L.case("icosphere"), L.case("bad_faces")
    np.testing.assert_array_equal(good['q'].view(np.uint32), bad['q'].view(np.uint32))
    rg, rb = run("icosphere"), run("bad_faces")
    assert rb['tree']['n'] == rg['tree']['n'] == 320 and rb['tree']['F'] == 322
    for k in ('w2', 'winf'):
        np.testing.assert_array_equal(rg[k].view(np.uint32), rb[k].view(np.uint32))
    np.testing.assert_array_equal(rg['sd']['signed'].view(np.uint32), rb['sd']['signed'].view(np.uint32))
    # the face indices are the input's: one face was inserted at 100
    fg, fb = rg['sd']['face'], rb['sd']['face']
    np.testing.assert_array_equal(np.where(fg >= 100, fg + 1, fg), fb)


def test_empty_mesh_and_no_queries():
    from customnerf_amd import mesh
    c, r = L.case("empty"), run("empty")
    assert r['tree']['n'] == 0 and (r['w2'] == 0).all() and (r['winf'] == 0).all() and r['stats2'] == (0, 0)
    assert (r['sd']['signed'] == np.inf).all() and (r['sd']['face'] == -1).all()
    bvh = mesh.build_bvh(cuda(L.case("icosphere")['v']), cuda(L.case("icosphere")['f']))
    none = torch.zeros(0, 3, device="cuda")
    assert mesh.winding_number(bvh, none).shape == (0,) and mesh.contains(bvh, none).dtype == torch.bool
    assert mesh.signed_distance(bvh, none)['signed'].shape == (0,)
    with pytest.raises(ValueError, match="points must be"):
        mesh.winding_number(bvh, torch.zeros(4, 2, device="cuda"))
    with pytest.raises(ValueError, match="beta"):
        mesh.signed_distance(bvh, torch.zeros(4, 3, device="cuda"), beta=0.0)


def test_far_field_prunes():
    c, r = L.case("torus"), run("torus")
    q = c['q'][:L.N_LATTICE]
    _, (accepted, tris) = gpu_winding(r['tree'], q, 2.0)
    n = c['tree']['n']
    print(f"torus lattice: {tris / len(q):.1f} triangles and {accepted / len(q):.1f} nodes per query of {n} faces")
    assert accepted > 0 and tris < len(q) * n / 4
    _, (a_inf, t_inf) = gpu_winding(r['tree'], q, math.inf)
    assert (a_inf, t_inf) == (0, len(q) * n)
