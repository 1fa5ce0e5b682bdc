"""NumPy restatement of mesh.topology and mesh.fill_holes, written from the rules of include/customnerf_hip.h (cnerf_mesh_topology*,
cnerf_mesh_holes_*) and not from the kernels of csrc/mesh_holes.hip.  Test infrastructure only.

Edges are classified by counting directed vertex pairs (np.unique), loops are found with a plain union-find over the boundary half-edges
of every vertex, and a loop is walked through a dictionary start vertex -> boundary half-edge.  The centroid and the normal of a fan are
float64 scalar operations, one rounding each, in the order the header writes them: the device results agree bit for bit.
"""
import numpy as np

from mesh_clean_restatement import labels

BAD_INDEX, NON_MANIFOLD, REPEATED = 1, 2, 4
INTERIOR, BOUNDARY, NONMAN = 1, 2, 3


def _faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("a face index lies outside [0, V)")
    return f


def classify(f, V):
    """per half-edge 3 f + k: (a, b, kind): 0 no edge (a == b), else INTERIOR / BOUNDARY / NONMAN by the counts of a -> b and b -> a"""
    a, b = f.ravel(), f[:, [1, 2, 0]].ravel()
    edge = a != b
    keys, cnt = np.unique((a * V + b)[edge], return_counts=True)

    def count(k):
        if not len(keys):
            return np.zeros(len(k), np.int64)
        i = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        return np.where(keys[i] == k, cnt[i], 0)
    same, opp = count(a * V + b), count(b * V + a)
    kind = np.where((same == 1) & (opp == 1), INTERIOR, np.where(same + opp == 1, BOUNDARY, NONMAN))
    return a, b, np.where(edge, kind, 0)


def loops(a, b, kind):
    """label (smallest half-edge id) of the loop of every boundary half-edge, -1 elsewhere"""
    parent = {int(h): int(h) for h in np.flatnonzero(kind == BOUNDARY)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    at = {}
    for h in parent:                                                            # boundary half-edges that touch a vertex form one loop
        for v in (int(a[h]), int(b[h])):
            if v in at:
                r0, r1 = find(at[v]), find(h)
                parent[max(r0, r1)] = min(r0, r1)
            else:
                at[v] = h
    lab = np.full(len(a), -1, np.int64)
    for h in parent:
        lab[h] = find(h)
    return lab


def _analyse(verts, faces):
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(v)
    f = _faces(faces, V)
    a, b, kind = classify(f, V)
    bnd = kind == BOUNDARY
    lab = loops(a, b, kind)
    pinched = (np.bincount(a[bnd], minlength=V) > 1) | (np.bincount(b[bnd], minlength=V) > 1)
    nm_end = np.zeros(V, bool)
    nm_end[a[kind == NONMAN]] = True
    nm_end[b[kind == NONMAN]] = True
    bad = pinched | nm_end
    ids = np.unique(lab[bnd])                                                    # increasing label
    length = np.array([int((lab == i).sum()) for i in ids], np.int32)
    simple = np.array([not (bad[a[lab == i]].any() or bad[b[lab == i]].any()) for i in ids], bool)
    return v, f, a, b, kind, pinched, ids, length, simple


def topology(verts, faces):
    """-> the dict of mesh.topology, loop_lengths as an int32 array"""
    v, f, a, b, kind, pinched, ids, length, simple = _analyse(verts, faces)
    V, F = len(v), len(f)
    und = np.minimum(a, b) * V + np.maximum(a, b)
    used = np.unique(f)
    t = {"vertices_used": len(used), "faces": F, "edges": len(np.unique(und[kind > 0])), "boundary_edges": int((kind == BOUNDARY).sum()),
         "nonmanifold_edges": len(np.unique(und[kind == NONMAN])), "pinched_vertices": int(pinched.sum()), "boundary_loops": len(ids),
         "simple_loops": int(simple.sum()), "components": len(np.unique(labels(f, V)[used])) if F else 0,
         "degenerate_faces": int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()), "loop_lengths": length}
    t["euler"] = t["vertices_used"] - t["edges"] + F
    t["watertight"] = F > 0 and not (t["boundary_edges"] or t["nonmanifold_edges"] or t["degenerate_faces"])
    return t


def fill_holes(verts, faces, normals=None, max_edges=None):
    """-> (verts, faces, normals or None, info) as mesh.fill_holes"""
    v, f, a, b, kind, _, ids, length, simple = _analyse(verts, faces)
    if (kind == NONMAN).any():
        raise ValueError("an edge lies in more than two faces or two faces use it in one direction")
    if (kind == 0).any():
        raise ValueError("a face repeats a vertex index")
    n_in = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    leaves = {int(a[h]): int(h) for h in np.flatnonzero(kind == BOUNDARY)}         # (unique per vertex on a simple loop: the only ones walked)
    new_v, new_n, new_f = [], [], []
    info = {"filled": 0, "skipped_pinched": int((~simple).sum()), "skipped_long": 0, "new_vertices": 0, "new_faces": 0}
    for h0, n, ok in zip(ids, length, simple):
        if not ok:
            continue
        if n < 3 or (max_edges is not None and n > max_edges):
            info["skipped_long"] += 1
            continue
        info["filled"] += 1
        walk, h = [], int(h0)
        for _ in range(n):
            walk.append((int(a[h]), int(b[h])))
            h = leaves[int(b[h])]
        assert h == int(h0)
        if n == 3:
            new_f.append([walk[0][1], walk[0][0], walk[1][1]])
            continue
        ci = len(v) + len(new_v)
        s = np.zeros(3, np.float64)
        for p, _ in walk:
            s = s + v[p].astype(np.float64)
        c = (s / np.float64(n)).astype(np.float32)
        new_v.append(c)
        new_f += [[q, p, ci] for p, q in walk]
        if n_in is not None:
            m = [np.float64(0.0)] * 3
            c64 = c.astype(np.float64)
            for p, q in walk:                                                    # the face (q, p, c): (p1 - p0) x (p2 - p0)
                pb = v[q].astype(np.float64)
                e1, e2 = v[p].astype(np.float64) - pb, c64 - pb
                m = [m[0] + (e1[1] * e2[2] - e1[2] * e2[1]), m[1] + (e1[2] * e2[0] - e1[0] * e2[2]), m[2] + (e1[0] * e2[1] - e1[1] * e2[0])]
            with np.errstate(all="ignore"):
                l = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                new_n.append(np.array([x / l for x in m], np.float64).astype(np.float32) if l > 0 else np.zeros(3, np.float32))
    info["new_vertices"], info["new_faces"] = len(new_v), len(new_f)
    vo = np.concatenate([v, np.array(new_v, np.float32).reshape(-1, 3)])
    fo = np.concatenate([f.astype(np.int32), np.array(new_f, np.int32).reshape(-1, 3)])
    no = None if n_in is None else np.concatenate([n_in, np.array(new_n, np.float32).reshape(-1, 3)])
    return vo, fo, no, info
