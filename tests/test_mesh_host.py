"""CPU: the marching-cubes table (csrc/mc_tables.h from csrc/gen_mc_tables.py), the NumPy restatement of mesh.hip on it, the PLY writer,
and the C-ABI of cnerf_marching_cubes_* up to the point where it would launch."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mc_restatement as R  # noqa: E402
from mc_restatement import gen_mc_tables as G  # noqa: E402

ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------------ table
def test_generator_reproduces_committed_header():
    with open(G.HEADER) as f:
        assert f.read() == G.header_text()
    assert subprocess.call([sys.executable, os.path.join(ROOT, "customnerf_amd", "csrc", "gen_mc_tables.py"), "--check"]) == 0


def test_case_bounds():
    tri, ntri = G.build()
    assert ntri.max() <= 5
    assert max(len(G.loops(c)) for c in range(256)) <= 4
    for c in range(256):
        assert (tri[c, 3 * ntri[c]:] == -1).all() and (tri[c, :3 * ntri[c]] >= 0).all()
    assert ntri[0] == 0 and ntri[255] == 0 and ntri[1] == 1


def crossing_edges(case):
    return {e for e, (a, b, _) in enumerate(G.EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}


def test_every_crossing_edge_in_exactly_one_loop():
    tri, ntri = G.build()
    for case in range(256):
        loops = G.loops(case)
        flat = [e for lp in loops for e in lp]
        assert sorted(flat) == sorted(crossing_edges(case)), case
        # and the table's triangles use exactly those edges
        assert set(tri[case, :3 * ntri[case]].tolist()) == crossing_edges(case), case


def face_cut(tri_row, n, face_edges):
    """directed triangle edges of one case whose two vertices lie on cube edges of one face"""
    out = set()
    for k in range(n):
        t = tri_row[3 * k:3 * k + 3]
        for q in range(3):
            a, b = int(t[q]), int(t[(q + 1) % 3])
            if a in face_edges and b in face_edges:
                out.add((a, b))
    return out


def test_complementary_face_cuts_agree():
    """cell A and its neighbour B across A's face (axis, side 1) = B's face (axis, side 0): whenever the four shared corners agree, the two
    cases draw the same segments on the face, in opposite directions (crack-free, consistently wound)."""
    tri, ntri = G.build()
    n_pairs = 0
    for axis in range(3):
        hi_corners = [c for c in range(8) if (c >> axis) & 1]
        hi_edges = {e for e, (a, b, ax) in enumerate(G.EDGES) if ax != axis and (a >> axis) & 1}
        to_lo = {e: G.EDGE_OF[frozenset((G.EDGES[e][0] & ~(1 << axis), G.EDGES[e][1] & ~(1 << axis)))] for e in hi_edges}
        lo_edges = set(to_lo.values())
        cuts_hi = [{(to_lo[a], to_lo[b]) for a, b in face_cut(tri[c], ntri[c], hi_edges)} for c in range(256)]
        cuts_lo = [face_cut(tri[c], ntri[c], lo_edges) for c in range(256)]
        for A in range(256):
            face_bits = [(A >> c) & 1 for c in hi_corners]
            for B in range(256):
                if [(B >> (c & ~(1 << axis))) & 1 for c in hi_corners] != face_bits:
                    continue
                n_pairs += 1
                assert cuts_hi[A] == {(b, a) for a, b in cuts_lo[B]}, (axis, A, B)
    assert n_pairs == 3 * 256 * 16


# ------------------------------------------------------------------------------------------------ restatement
def lattice(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    sp = float(x[1] - x[0])
    return X, Y, Z, (sp, sp, sp), (lo, lo, lo)


def test_restatement_sphere_closed_outward():
    X, Y, Z, sp, org = lattice(24)
    vol = (1 - np.sqrt(X ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)          # value >= 0.4 inside a sphere of radius 0.6
    v, f, n = R.marching_cubes(vol, 0.4, sp, org)
    assert len(f) > 100 and (len(v), len(f)) == R.counts(vol, 0.4)
    assert R.check_closed_oriented(v, f) == 0
    assert R.euler_characteristic(v, f) == 2
    r = np.linalg.norm(v, axis=1)
    assert np.abs(r - 0.6).max() < sp[0]
    fn = R.face_normals(v, f)
    assert ((fn * v[f].mean(1)).sum(1) > 0).all()                              # wound from inside to outside
    assert ((n * v).sum(1) > 0).all() and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)


def test_restatement_touching_spheres():
    X, Y, Z, sp, org = lattice(25, -1.2, 1.2)                                   # x = 0 is a lattice plane: the spheres touch there
    vol = np.maximum(0.5 - np.sqrt((X - 0.5) ** 2 + Y ** 2 + Z ** 2), 0.5 - np.sqrt((X + 0.5) ** 2 + Y ** 2 + Z ** 2)).astype(np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, sp, org)
    assert R.check_closed_oriented(v, f) == 0
    assert R.euler_characteristic(v, f) in (2, 4)                             # one merged surface or two spheres, either way closed


@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_noise_manifold(seed):
    vol = np.random.default_rng(seed).random((20, 20, 20), dtype=np.float32)
    v, f, _ = R.marching_cubes(vol, 0.5)
    assert len(f) > 10000
    assert R.check_closed_oriented(v, f, box_lo=[0, 0, 0], box_hi=[19, 19, 19]) > 0


def test_restatement_nan_is_outside():
    vol = np.zeros((3, 3, 3), dtype=np.float32)
    vol[1, 1, 1] = np.nan
    assert R.counts(vol, 0.0)[0] == 6                                          # the NaN point is outside: its 6 edges cross
    v, f, _ = R.marching_cubes(vol, 0.0)
    assert R.check_closed_oriented(v, f) == 0 and len(f) == 8


# ------------------------------------------------------------------------------------------------ PLY
def test_write_ply_round_trip(tmp_path):
    from customnerf_amd import mesh
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3)).astype(np.int32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    c = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    p = str(tmp_path / "m.ply")
    mesh.write_ply(p, v, f, normals=n, colors=c)
    back = R.read_ply(p)
    assert np.array_equal(back["verts"], v) and np.array_equal(back["faces"], f)
    assert np.array_equal(back["normals"], n) and np.array_equal(back["colors"], c)
    head = open(p, "rb").read().split(b"end_header\n")[0].decode()
    assert head == ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                    "element face 5\nproperty list uchar int vertex_indices\n")
    size = os.path.getsize(p) - len(head) - len("end_header\n")
    assert size == 7 * (24 + 3) + 5 * 13
    p2 = str(tmp_path / "plain.ply")
    mesh.write_ply(p2, v, f)
    back = R.read_ply(p2)
    assert set(back) == {"verts", "faces"} and np.array_equal(back["verts"], v)
    assert b"property float nx" not in open(p2, "rb").read()


# ------------------------------------------------------------------------------------------------ C-ABI
def test_abi_declared_and_bound():
    from customnerf_amd import _lib
    src = open(os.path.join(ROOT, "include", "customnerf_hip.h")).read()
    for name in ("cnerf_marching_cubes_workspace_bytes", "cnerf_marching_cubes_count", "cnerf_marching_cubes_emit"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 8 and _lib.lib.cnerf_abi_version() == 8


def test_workspace_bytes():
    from customnerf_amd import mesh
    for n in (2, 33, 512):
        assert mesh.workspace_bytes((n, n, n)) <= 6.1 * n ** 3 + 5 * 256          # (sections are 256-byte aligned)
    assert mesh.workspace_bytes((512, 512, 512)) / 512 ** 3 <= 6.1
    assert mesh.workspace_bytes((33, 17, 9)) >= 6 * 33 * 17 * 9
    # pinned: callers size their buffers by these (the last shape is the largest accepted)
    for shape, b in (((2, 2, 2), 1280), ((33, 17, 9), 30976), ((33, 33, 33), 217600), ((512, 512, 512), 809500928),
                     ((2047, 1024, 1024), 12945686784)):
        assert mesh.workspace_bytes(shape) == b


def test_argument_checks_reject_before_launch():
    from customnerf_amd._lib import lib
    EINVAL, ENULL = -1, -2
    out = C.c_uint64(0)
    assert lib.cnerf_marching_cubes_workspace_bytes(1, 4, 4, C.byref(out)) == EINVAL
    assert lib.cnerf_marching_cubes_workspace_bytes(2048, 1024, 1024, C.byref(out)) == EINVAL        # 2^31 points
    assert lib.cnerf_marching_cubes_workspace_bytes(4, 4, 4, None) == ENULL
    assert lib.cnerf_marching_cubes_workspace_bytes(4, 4, 4, C.byref(out)) == 0 and out.value > 0
    ws_bytes = out.value
    fake = 1 << 20                                   # never dereferenced: every call below is rejected first
    assert lib.cnerf_marching_cubes_count(fake, 4, 4, 1, 0.0, fake, ws_bytes, fake, None) == EINVAL
    assert lib.cnerf_marching_cubes_count(None, 4, 4, 4, 0.0, fake, ws_bytes, fake, None) == ENULL
    assert lib.cnerf_marching_cubes_count(fake, 4, 4, 4, 0.0, None, ws_bytes, fake, None) == ENULL
    assert lib.cnerf_marching_cubes_count(fake, 4, 4, 4, 0.0, fake, ws_bytes, None, None) == ENULL
    assert lib.cnerf_marching_cubes_count(fake, 4, 4, 4, 0.0, fake, ws_bytes - 1, fake, None) == EINVAL   # short workspace
    assert lib.cnerf_marching_cubes_count(fake, 4, 4, 4, 0.0, fake + 4, ws_bytes, fake, None) == EINVAL   # misaligned workspace
    f3 = (C.c_float * 3)(0, 0, 0)
    s3 = (C.c_float * 3)(1, 1, 1)
    emit = lib.cnerf_marching_cubes_emit
    assert emit(fake, 4, 4, 4, 0.0, f3, s3, fake, ws_bytes - 1, fake, None, fake, 1, 1, None) == EINVAL
    assert emit(fake, 1 << 16, 1 << 15, 2, 0.0, f3, s3, fake, ws_bytes, fake, None, fake, 1, 1, None) == EINVAL
    assert emit(fake, 4, 4, 4, 0.0, None, s3, fake, ws_bytes, fake, None, fake, 1, 1, None) == ENULL
    assert emit(fake, 4, 4, 4, 0.0, f3, None, fake, ws_bytes, fake, None, fake, 1, 1, None) == ENULL
    assert emit(fake, 4, 4, 4, 0.0, f3, s3, fake, ws_bytes, None, None, fake, 1, 1, None) == ENULL       # verts with max_verts > 0
    assert emit(fake, 4, 4, 4, 0.0, f3, s3, fake, ws_bytes, fake, None, None, 1, 1, None) == ENULL       # faces with max_faces > 0
