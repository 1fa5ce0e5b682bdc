"""NumPy restatement of csrc/mesh_decimate.hip (quadric edge-collapse decimation), rule for rule and vectorised over edges.  Test
infrastructure only.

Every float operation is a separate float64 ufunc (+ - * / sqrt), correctly rounded and never fused, in the order the kernels write it, and
the kernels are built with -ffp-contract=off: costs, keys and positions agree bit for bit.  The Jacobi sweep is restated as written (no
np.linalg.eigh).  Where the kernels use atomics (degrees, minima, list slots), the result does not depend on their order, and the
restatement computes it directly: np.minimum.at for the minima, a sort for the radix select.
"""
import numpy as np

MAX_DEG = 32
EIG_CUT = 1e-3
FLIP = 0.2
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)
BAD_INDEX, NON_MANIFOLD, REPEATED = 1, 2, 4


def face_quadrics(P, faces):
    """[F, 10] (A00 A01 A02 A11 A12 A22 b0 b1 b2 c) of area (n n^T, n d, d^2) and [F] bool: nonzero, finite area"""
    p = P.astype(np.float64)[faces]                                              # [F, 3, 3]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    m = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    with np.errstate(all="ignore"):
        mm = np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
        good = (mm > 0) & (mm < 1e300)
        n = [m[a] / mm for a in range(3)]
        area = 0.5 * mm
        d = np.zeros(len(faces))
        for a in range(3):
            d = d - n[a] * p[:, 0, a]
        q = np.stack([area * n[0] * n[0], area * n[0] * n[1], area * n[0] * n[2], area * n[1] * n[1], area * n[1] * n[2], area * n[2] * n[2],
                      area * n[0] * d, area * n[1] * d, area * n[2] * d, area * d * d], 1)
    return q, good


def jacobi(s):
    """mesh_qef.h qef_jacobi over [C, 6] -> (w [C, 3], v [C, 3, 3])"""
    C = len(s)
    a = np.stack([s[:, [0, 1, 2]], s[:, [1, 3, 4]], s[:, [2, 4, 5]]], 1).copy()
    v = np.tile(np.eye(3), (C, 1, 1))
    act = np.ones(C, bool)
    with np.errstate(all="ignore"):
        for _ in range(32):
            off = a[:, 0, 1] * a[:, 0, 1] + a[:, 0, 2] * a[:, 0, 2] + a[:, 1, 2] * a[:, 1, 2]
            dia = a[:, 0, 0] * a[:, 0, 0] + a[:, 1, 1] * a[:, 1, 1] + a[:, 2, 2] * a[:, 2, 2]
            act &= off > 1e-36 * dia
            if not act.any():
                break
            for pq in range(3):
                p, q = (1 if pq == 2 else 0), (1 if pq == 0 else 2)
                apq = a[:, p, q]
                do = act & (apq != 0.0)
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                for k in range(3):
                    akp, akq = a[:, k, p].copy(), a[:, k, q].copy()
                    a[:, k, p] = np.where(do, c * akp - sn * akq, akp)
                    a[:, k, q] = np.where(do, sn * akp + c * akq, akq)
                for k in range(3):
                    apk, aqk = a[:, p, k].copy(), a[:, q, k].copy()
                    a[:, p, k] = np.where(do, c * apk - sn * aqk, apk)
                    a[:, q, k] = np.where(do, sn * apk + c * aqk, aqk)
                for k in range(3):
                    vkp, vkq = v[:, k, p].copy(), v[:, k, q].copy()
                    v[:, k, p] = np.where(do, c * vkp - sn * vkq, vkp)
                    v[:, k, q] = np.where(do, sn * vkp + c * vkq, vkq)
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1), v


def qef_solve(s, b, xb):
    """mesh_qef.h qef_solve: x = xb + A+ (-b - A xb) over [C] rows"""
    w, v = jacobi(s)
    wmax = np.fmax(w[:, 0], np.fmax(w[:, 1], w[:, 2]))
    r = [-b[:, 0] - (s[:, 0] * xb[:, 0] + s[:, 1] * xb[:, 1] + s[:, 2] * xb[:, 2]),
         -b[:, 1] - (s[:, 1] * xb[:, 0] + s[:, 3] * xb[:, 1] + s[:, 4] * xb[:, 2]),
         -b[:, 2] - (s[:, 2] * xb[:, 0] + s[:, 4] * xb[:, 1] + s[:, 5] * xb[:, 2])]
    x = xb.copy()
    with np.errstate(all="ignore"):
        for e in range(3):
            keep = (wmax > 0.0) & (w[:, e] >= EIG_CUT * wmax)
            c = (v[:, 0, e] * r[0] + v[:, 1, e] * r[1] + v[:, 2, e] * r[2]) / w[:, e]
            for j in range(3):
                x[:, j] = np.where(keep, x[:, j] + c * v[:, j, e], x[:, j])
    return x


def lists(faces, V):
    """(degree [V], padded vertex -> face lists [V, D] (-1: none), increasing face index)"""
    flat = faces.ravel()
    deg = np.bincount(flat, minlength=V)
    order = np.argsort(flat, kind="stable")
    vs = flat[order]
    start = np.cumsum(deg) - deg
    D = int(deg.max()) if len(flat) else 0
    L = np.full((V, max(D, 1)), -1, np.int64)
    L[vs, np.arange(len(flat)) - start[vs]] = order // 3
    return deg, L


def twins(faces, V):
    """twin half-edge of every half-edge 3 f + k (-1: none) and the count of each directed edge"""
    a = faces.ravel()
    b = faces[:, [1, 2, 0]].ravel()
    code, rev = a * V + b, b * V + a
    srt = np.argsort(code, kind="stable")
    cs = code[srt]
    i = np.searchsorted(cs, rev)
    ic = np.minimum(i, max(len(cs) - 1, 0))
    found = (i < len(cs)) & (cs[ic] == rev) if len(cs) else np.zeros(0, bool)
    tw = np.where(found, srt[ic] if len(cs) else 0, -1)
    _, cnt = np.unique(code, return_counts=True)
    return tw, a, b, cnt


def init(verts, faces):
    """-> state dict, flags (the kernels' bits)"""
    P = np.array(verts, dtype=np.float32).reshape(-1, 3)
    V = len(P)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    flags = 0
    ok = ((f >= 0) & (f < V)).all(axis=1)
    if not ok.all():
        flags |= BAD_INDEX
    fv = f[ok]
    if ((fv[:, 0] == fv[:, 1]) | (fv[:, 1] == fv[:, 2]) | (fv[:, 0] == fv[:, 2])).any():
        flags |= REPEATED
    if flags:
        return None, flags
    deg, L = lists(f, V)
    _, _, _, cnt = twins(f, V)
    if (cnt > 1).any():
        flags |= NON_MANIFOLD
    fq, good = face_quadrics(P, f)
    Q = np.zeros((V, 10))
    for k in range(L.shape[1]):
        sel = np.flatnonzero(deg > k)
        g = L[sel, k]
        add = good[g]
        Q[sel[add]] = Q[sel[add]] + fq[g[add]]
    return {"P": P, "Q": Q, "faces": f, "refs": int((deg > 0).sum())}, flags


def _others(faces, L, c):
    """[C, 2D]: the other two vertices of each face in the lists L [C, D] of the centres c, in face order from c; -1 for no face"""
    fv = faces[np.maximum(L, 0)]                                                 # [C, D, 3]
    j = np.argmax(fv == c[:, None, None], axis=2)
    o1 = np.take_along_axis(fv, ((j + 1) % 3)[..., None], 2)[..., 0]
    o2 = np.take_along_axis(fv, ((j + 2) % 3)[..., None], 2)[..., 0]
    o = np.stack([o1, o2], 2)
    o[L < 0] = -1
    return o.reshape(len(c), 2 * L.shape[1])


def _cross(p):
    e1, e2 = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :]
    return [e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
            e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]]


def place(st, bnd, u, v):
    """dc_place: (kept, removed, Q [C, 10], x f64 [C, 3], cost f32 [C])"""
    P, Q = st["P"], st["Q"]
    Qs = Q[u] + Q[v]
    bu, bv = bnd[u], bnd[v]
    kept = np.where(bu, u, np.where(bv, v, u))
    removed = np.where(bu, v, np.where(bv, u, v))
    m = (P[u].astype(np.float64) + P[v].astype(np.float64)) * 0.5
    x = qef_solve(Qs[:, :6], Qs[:, 6:9], m)
    x = np.where((bu | bv)[:, None], P[kept].astype(np.float64), x)
    s = Qs
    with np.errstate(all="ignore"):
        ax = [s[:, 0] * x[:, 0] + s[:, 1] * x[:, 1] + s[:, 2] * x[:, 2], s[:, 1] * x[:, 0] + s[:, 3] * x[:, 1] + s[:, 4] * x[:, 2],
              s[:, 2] * x[:, 0] + s[:, 4] * x[:, 1] + s[:, 5] * x[:, 2]]
        xax = x[:, 0] * ax[0] + x[:, 1] * ax[1] + x[:, 2] * ax[2]
        bx = s[:, 6] * x[:, 0] + s[:, 7] * x[:, 1] + s[:, 8] * x[:, 2]
        cost = xax + 2.0 * bx + s[:, 9]
        cost = np.where(cost > 0.0, cost, 0.0).astype(np.float32)
    return kept, removed, Qs, x, cost


def round_(st, target):
    """one round in place -> (referenced vertices, faces, collapses)"""
    P, f = st["P"], st["faces"]
    V, F = len(P), len(f)
    if F == 0:
        return st["refs"], 0, 0
    deg, L = lists(f, V)
    tw, a, b, _ = twins(f, V)
    bnd = np.zeros(V, bool)
    bnd[a[tw < 0]] = True
    bnd[b[tw < 0]] = True
    ci = np.flatnonzero((tw >= 0) & (a < b) & ~(bnd[a] & bnd[b]) & (deg[a] <= MAX_DEG) & (deg[b] <= MAX_DEG))
    u, v, fe, ge = a[ci], b[ci], ci // 3, tw[ci] // 3
    D = int(max(deg[u].max(), deg[v].max())) if len(ci) else 1
    Lu, Lv = L[u, :D], L[v, :D]
    # link condition: exactly two distinct shared neighbours
    Nu, Nv = _others(f, Lu, u), _others(f, Lv, v)
    in_u = (Nv[:, :, None] == Nu[:, None, :]).any(2) & (Nv >= 0) & (Nv != u[:, None])
    srt = np.sort(np.where(in_u, Nv, -1), axis=1)
    common = ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] >= 0)).sum(1) + (srt[:, 0] >= 0)
    link = common == 2
    # surviving faces around u then v
    S = np.concatenate([Lu, Lv], 1)                                             # [C, 2D]
    cen = np.concatenate([np.repeat(u[:, None], D, 1), np.repeat(v[:, None], D, 1)], 1)
    surv = (S >= 0) & (S != fe[:, None]) & (S != ge[:, None])
    fv = f[np.maximum(S, 0)]                                                    # [C, 2D, 3]
    j = np.argmax(fv == cen[..., None], axis=2)
    x0 = np.take_along_axis(fv, ((j + 1) % 3)[..., None], 2)[..., 0]
    x1 = np.take_along_axis(fv, ((j + 2) % 3)[..., None], 2)[..., 0]
    pair = np.where(surv, np.minimum(x0, x1) * V + np.maximum(x0, x1), -1 - np.arange(2 * D)[None, :])
    ps = np.sort(pair, axis=1)
    distinct = ~((ps[:, 1:] == ps[:, :-1]) & (ps[:, 1:] >= 0)).any(1)
    # position, cost
    kept, removed, Qs, x, cost = place(st, bnd, u, v)
    Pk = x.astype(np.float32)
    # normal flips of the surviving faces
    po = P.astype(np.float64)[fv]                                               # [C, 2D, 3, 3]
    moved = (fv == u[:, None, None]) | (fv == v[:, None, None])
    pn = np.where(moved[..., None], Pk.astype(np.float64)[:, None, None, :], po)
    no, nw = _cross(po), _cross(pn)
    with np.errstate(all="ignore"):
        nno = no[0] * no[0] + no[1] * no[1] + no[2] * no[2]
        nnw = nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]
        dot = nw[0] * no[0] + nw[1] * no[1] + nw[2] * no[2]
        flip = surv & (nno > 0.0) & (dot <= FLIP * np.sqrt(nnw) * np.sqrt(nno))
    valid = link & distinct & ~flip.any(1)
    key = (cost.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ci.astype(np.uint64)
    key = np.where(valid, key, NOKEY)
    # independent selection
    vkey = np.full(V, NOKEY, np.uint64)
    np.minimum.at(vkey, u[valid], key[valid])
    np.minimum.at(vkey, v[valid], key[valid])
    pre = valid & (vkey[u] == key) & (vkey[v] == key)
    hood = f[np.maximum(S, 0)]                                                  # every vertex of every face around u or v
    hmask = np.repeat((S >= 0)[..., None], 3, 2)
    nkey = np.full(V, NOKEY, np.uint64)
    kb = np.broadcast_to(key[:, None, None], hood.shape)
    np.minimum.at(nkey, hood[pre][hmask[pre]], kb[pre][hmask[pre]])
    win = pre & np.where(hmask, nkey[hood] == key[:, None, None], True).all((1, 2))
    W = int(win.sum())
    n = W
    if F < target + 2 * W:
        n = (F - target + 1) // 2 if F > target else 0
    wi = np.flatnonzero(win)
    wi = wi[np.argsort(key[wi])][:n]
    # apply
    st["P"][kept[wi]] = Pk[wi]
    st["Q"][kept[wi]] = Qs[wi]
    remap = np.arange(V)
    remap[removed[wi]] = kept[wi]
    dead = np.zeros(F, bool)
    dead[fe[wi]] = True
    dead[ge[wi]] = True
    st["faces"] = remap[f[~dead]]
    st["refs"] -= n
    return st["refs"], len(st["faces"]), n


def emit(st, normals=None):
    f = st["faces"]
    V = len(st["P"])
    old = np.unique(f)
    new = np.full(V, -1, np.int64)
    new[old] = np.arange(len(old))
    no = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)[old]
    return st["P"][old], new[f].astype(np.int32).reshape(-1, 3), no, old.astype(np.int32)


def decimate(verts, faces, target_faces, normals=None):
    """-> (verts, faces, normals, old_index, rounds [(referenced vertices, faces, collapses)]) as mesh.decimate; ValueError on the flags"""
    st, flags = init(verts, faces)
    if flags:
        raise ValueError(f"decimate: flags {flags}")
    rounds = []
    while len(st["faces"]) > target_faces:
        r = round_(st, target_faces)
        rounds.append(r)
        if r[2] == 0:
            break
    return emit(st, normals) + (rounds,)


def check_manifold(faces):
    """every undirected edge in one or two faces, two only in opposite directions; no repeated index.  -> number of boundary edges"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    V = int(f.max()) + 1 if len(f) else 0
    tw, _, _, cnt = twins(f, V)
    assert (cnt == 1).all()
    return int((tw < 0).sum())


def euler(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return len(np.unique(f)) - len(np.unique(e, axis=0)) + len(f)
