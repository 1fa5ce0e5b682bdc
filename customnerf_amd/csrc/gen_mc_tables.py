"""Generates mc_tables.h, the marching-cubes case table of mesh.hip (run by hand after a change; the build runs no Python).

Cube conventions (shared with mesh.hip and the NumPy restatement in tests/mc_restatement.py):
  corner c = dx | dy << 1 | dz << 2   (dx, dy, dz in {0, 1} along the volume's axes 0, 1, 2; axis 2 is the fastest in memory)
  edge   e = 4 * axis + k, k = 0..3: the edge along `axis` whose lower corner is the k-th corner (in increasing order) with bit `axis` clear
  case     = sum over inside corners of 1 << c   (inside <=> value >= level)

The table comes from a rule on the six faces, not from a list typed by hand:
  * on each face the crossing edges are joined into segments; a face with two diagonal inside corners gives each inside corner its own
    segment ("separate inside"), so the cut of a face depends on that face's four corners only and two cells sharing it cut it alike;
  * every segment is directed by the right-hand rule, T = g x n_f (g = in-face direction from the inside towards the outside corners,
    n_f = the face's outward normal), so the two cells on either side of a face run a shared segment in opposite directions;
  * the directed segments chain into closed loops; each loop is fan-triangulated from its lowest edge whose diagonals do not join two
    edges of one face (a loop that crosses an ambiguous face twice would otherwise draw a chord in that face, and the neighbouring cell
    can draw the same one: four triangles on one mesh edge), and the loop's direction makes (v1 - v0) x (v2 - v0) point from inside to
    outside.  Every mesh edge in a cube face is then a segment of that face, shared with the neighbour.
The generator asserts the bounds mesh.hip relies on: at most 5 triangles and 4 loops per case.

    python gen_mc_tables.py            # rewrites mc_tables.h next to this file
    python gen_mc_tables.py --check    # exit status 1 if mc_tables.h differs from what the rule gives
"""
import os
import sys

import numpy as np

MAX_TRIS = 5
MAX_LOOPS = 4


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edges():
    """[12] (corner a, corner b, axis) with a < b, b = a | 1 << axis"""
    out = []
    for axis in range(3):
        lows = [c for c in range(8) if not (c >> axis) & 1]
        out += [(c, c | (1 << axis), axis) for c in lows]
    return out


EDGES = edges()
EDGE_OF = {frozenset((a, b)): e for e, (a, b, _) in enumerate(EDGES)}


def faces():
    """[6] (cyclic list of 4 corners, outward normal)"""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = side << axis
            ring = [base, base | 1 << u, base | 1 << u | 1 << v, base | 1 << v]
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            out.append((ring, n))
    return out


FACES = faces()


def face_segments(case, ring):
    """undirected segments (pairs of edges) of one face: depends on the face's four corners only"""
    ins = [(case >> c) & 1 for c in ring]
    ring_edges = [EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))] for i in range(4)]   # edge i joins ring[i] and ring[i+1]
    n_in = sum(ins)
    if n_in in (0, 4):
        return []
    if n_in == 2 and ins[0] == ins[2]:                       # ambiguous face: separate inside corners
        return [(ring_edges[(i - 1) % 4], ring_edges[i]) for i in range(4) if ins[i]]
    crossing = [ring_edges[i] for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    assert len(crossing) == 2
    return [tuple(crossing)]


def inside_to_outside(case, e):
    a, b, _ = EDGES[e]
    d = corner_pos(b) - corner_pos(a)
    return d if (case >> a) & 1 else -d


def mid(e):
    a, b, _ = EDGES[e]
    return 0.5 * (corner_pos(a) + corner_pos(b))


def directed_segments(case):
    segs = []
    for ring, n in FACES:
        for e0, e1 in face_segments(case, ring):
            g = inside_to_outside(case, e0) + inside_to_outside(case, e1)
            t = np.cross(g, n)
            d = float(np.dot(mid(e1) - mid(e0), t))
            assert d != 0.0
            segs.append((e0, e1) if d > 0 else (e1, e0))
    return segs


def loops(case):
    nxt = {}
    for a, b in directed_segments(case):
        assert a not in nxt, f"case {case}: edge {a} leaves two segments"
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), f"case {case}: segments do not close"
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        out.append(loop)                                     # starts at its lowest edge (loops are visited from their lowest edge)
    return out


FACE_EDGES = [{EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))] for i in range(4)} for ring, _ in FACES]


def in_face_chord(a, b):
    """edges a and b lie on one cube face: a fan diagonal between them would lie in that face, where the neighbouring cell may draw the
    same chord (four triangles on one mesh edge)"""
    return any(a in fe and b in fe for fe in FACE_EDGES)


def fan_apex(loop):
    """position of the fan's apex in `loop`: its lowest edge whose diagonals avoid in-face chords (a loop that crosses an ambiguous face
    twice has such chords from some of its vertices)"""
    n = len(loop)
    for k in sorted(range(n), key=lambda k: loop[k]):
        if not any(in_face_chord(loop[k], loop[(k + i) % n]) for i in range(2, n - 1)):
            return k
    raise AssertionError(f"loop {loop}: every fan has an in-face chord")


def triangles(case):
    tris = []
    for loop in loops(case):
        assert len(loop) >= 3
        k = fan_apex(loop)
        loop = loop[k:] + loop[:k]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def build():
    """-> (tri [256][16] int8, -1 padded; ntri [256] uint8)"""
    tri = np.full((256, 16), -1, dtype=np.int8)
    ntri = np.zeros(256, dtype=np.uint8)
    for case in range(256):
        ls = loops(case)
        ts = triangles(case)
        assert len(ls) <= MAX_LOOPS, f"case {case}: {len(ls)} loops"
        assert len(ts) <= MAX_TRIS, f"case {case}: {len(ts)} triangles"
        for k, t in enumerate(ts):
            tri[case, 3 * k:3 * k + 3] = t
        ntri[case] = len(ts)
    return tri, ntri


def header_text():
    tri, ntri = build()
    lines = ["// Generated by gen_mc_tables.py — do not edit; rerun the script after changing the rule.",
             "// Marching-cubes case table of mesh.hip: face rule 'separate inside' on ambiguous faces, loops fan-triangulated without in-face",
             "// chords, winding (v1 - v0) x (v2 - v0) from inside (value >= level) to outside.  Conventions and rule: gen_mc_tables.py.",
             "// Device tables (__constant__): included by mesh.hip only.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             f"#define CN_MC_MAX_TRIS {MAX_TRIS}",
             "",
             "// edge e -> (lower corner, axis); the upper corner is lower | 1 << axis",
             "static __constant__ const uint8_t cn_mc_edge_corner[12] = {" + ", ".join(str(a) for a, _, _ in EDGES) + "};",
             "static __constant__ const uint8_t cn_mc_edge_axis[12] = {" + ", ".join(str(ax) for _, _, ax in EDGES) + "};",
             "",
             "// triangles per case",
             "static __constant__ const uint8_t cn_mc_ntri[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(v)) for v in ntri[r:r + 32]) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"// edges of the triangles of each case, 3 per triangle, -1 padded ({MAX_TRIS} triangles at most)")
    lines.append("static __constant__ const int8_t cn_mc_tri[256][16] = {")
    for case in range(256):
        lines.append("    {" + ", ".join(str(int(v)) for v in tri[case]) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mc_tables.h")

if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        with open(HEADER) as f:
            sys.exit(0 if f.read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
