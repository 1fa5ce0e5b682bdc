"""NumPy restatement of csrc/mesh_smooth.hip (Taubin smoothing with uniform weights, area-weighted vertex normals), rule for rule and
vectorised over vertices.  Test infrastructure only.

Every float operation is a separate float32 ufunc (+ - * / sqrt), correctly rounded and never fused, in the order the kernels write it, and
the kernels are built with -ffp-contract=off: positions agree bit for bit.  The kernels fill their lists with atomics and sort them before
reading them; the restatement builds the sorted lists directly.
"""
import numpy as np

BAD_INDEX = 1
MAX_F = 0x2AAAAAAA


def _padded(owner, item, V):
    """rows of `item` grouped by `owner` (both sorted by (owner, item)) -> (count [V], padded [V, D] (-1: none))"""
    cnt = np.bincount(owner, minlength=V).astype(np.int64)
    start = np.cumsum(cnt) - cnt
    L = np.full((V, max(int(cnt.max()) if V else 0, 1)), -1, np.int64)
    if len(owner):
        L[owner, np.arange(len(owner)) - start[owner]] = item
    return cnt, L


def lists(faces, V):
    """-> dict(flags, nbr [V, D] sorted distinct neighbours (-1 pad), count [V], boundary [V] bool, flist [V, E] sorted faces, fcount [V]),
    or dict(flags=BAD_INDEX) alone"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not ((f >= 0) & (f < V)).all():
        return {"flags": BAD_INDEX}
    F = len(f)
    fid = np.repeat(np.arange(F), 3)
    a, b = f.ravel(), f[:, [1, 2, 0]].ravel()
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    # distinct undirected edges of each face
    e = np.unique(np.stack([fid[keep], lo[keep], hi[keep]], 1), axis=0) if keep.any() else np.zeros((0, 3), np.int64)
    owner = np.concatenate([e[:, 1], e[:, 2]])
    other = np.concatenate([e[:, 2], e[:, 1]])
    pairs, mult = (np.unique(np.stack([owner, other], 1), axis=0, return_counts=True) if len(owner)
                   else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))
    count, nbr = _padded(pairs[:, 0], pairs[:, 1], V)
    boundary = np.zeros(V, bool)
    boundary[pairs[mult == 1, 0]] = True
    # distinct vertices of each face -> vertex -> face lists in increasing face index
    vf = np.unique(np.stack([f.ravel(), fid], 1), axis=0) if F else np.zeros((0, 2), np.int64)
    fcount, flist = _padded(vf[:, 0], vf[:, 1], V)
    return {"flags": 0, "nbr": nbr, "count": count, "boundary": boundary, "flist": flist, "fcount": fcount}


def step(P, L, s, pin_boundary=True):
    """one Jacobi step with factor s (float32) of positions P [V, 3] float32 over the lists L"""
    cnt = L["count"]
    move = cnt > 0
    if pin_boundary:
        move &= ~L["boundary"]
    out = P.copy()
    if not move.any():
        return out
    nbr = L["nbr"][move]
    c = cnt[move]
    acc = P[nbr[:, 0]].copy()
    for i in range(1, nbr.shape[1]):
        m = c > i
        acc[m] = acc[m] + P[nbr[m, i]]
    mean = acc / c.astype(np.float32)[:, None]
    x = P[move]
    out[move] = x + np.float32(s) * (mean - x)
    return out


def smooth(verts, faces, iterations=10, lamb=0.5, mu=-0.53, pin_boundary=True, normals=None):
    """mesh.smooth -> (verts [V, 3] float32, normals [V, 3] float32); ValueError on a bad index"""
    P = np.array(verts, dtype=np.float32).reshape(-1, 3)
    L = lists(faces, len(P))
    if L["flags"]:
        raise ValueError("a face index lies outside [0, V)")
    lamb, mu = np.float32(lamb), np.float32(mu)
    for _ in range(int(iterations)):
        P = step(P, L, lamb, pin_boundary)
        if mu != 0:
            P = step(P, L, mu, pin_boundary)
    return P, vertex_normals(P, faces, normals, L)


def face_normals(P, faces):
    """(p1 - p0) x (p2 - p0) per face in float32, the kernels' component order"""
    p = P[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def vertex_normals(verts, faces, normals=None, L=None):
    """mesh.vertex_normals: the face normals of each vertex added to zero in increasing face index, normalised; the input normal (or zero)
    where the squared length is not in (0, inf)"""
    P = np.array(verts, dtype=np.float32).reshape(-1, 3)
    V = len(P)
    if L is None:
        L = lists(faces, V)
        if L["flags"]:
            raise ValueError("a face index lies outside [0, V)")
    c = face_normals(P, faces)
    acc = np.zeros((V, 3), np.float32)
    fl, fc = L["flist"], L["fcount"]
    for i in range(fl.shape[1]):
        m = fc > i
        acc[m] = acc[m] + c[fl[m, i]]
    with np.errstate(all="ignore"):
        q = acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2]
        ok = (q > 0) & (q < np.inf)
        r = np.sqrt(q)
        out = acc / r[:, None]
    fallback = np.zeros((V, 3), np.float32) if normals is None else np.array(normals, dtype=np.float32).reshape(-1, 3)
    return np.where(ok[:, None], out, fallback).astype(np.float32)
