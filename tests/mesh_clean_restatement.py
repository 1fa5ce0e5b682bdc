"""NumPy restatement of csrc/mesh_clean.hip (component removal, vertex clustering).  Test infrastructure only.

Components: labels by min-label propagation over the faces with pointer jumping (the smallest vertex index of each component, which the
kernels' min-root union-find also gives), face counts on the label of each face's first vertex, selection and order-keeping compaction.
Clustering: cells by the kernels' float32 formula, clusters in linear cell order, faces deduplicated by first occurrence of their unordered
cluster triple; the fixed-point sums are restated term by term (float64, rounded to the kernels' scales) and the representative is solved
with np.linalg.eigh.  cluster() also returns the clusters whose eigenvalue ratio lies within 2x of the cutoff, where a last-bit difference
between the two eigen-solvers may keep or drop an eigenvalue: tests leave those out of the position comparison.
"""
import numpy as np

SP, SN, SQ = 2.0 ** 24, 2.0 ** 28, 2.0 ** 32
EIG_CUT = 1e-3


def _check_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("a face index lies outside [0, V)")
    return f


def labels(faces, V):
    """label[v] = smallest vertex index of v's component (vertices joined by a face)"""
    f = _check_faces(faces, V)
    lab = np.arange(V, dtype=np.int64)
    while True:
        prev = lab.copy()
        m = lab[f].min(axis=1) if len(f) else np.zeros(0, np.int64)
        for q in range(3):
            np.minimum.at(lab, f[:, q], m)
        while True:                                                              # pointer jumping
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, prev):
            return lab


def components(verts, faces, normals=None, min_faces=1, largest=False):
    """-> (verts, faces, normals, old_index) as mesh.remove_small_components"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(v)
    f = _check_faces(faces, V)
    lab = labels(f, V)
    fcount = np.bincount(lab[f[:, 0]], minlength=V) if len(f) else np.zeros(V, np.int64)
    keep = fcount >= min_faces
    if largest:
        big = int(np.argmax(fcount)) if V else 0                                  # first maximum = smallest label on a tie
        keep &= (np.arange(V) == big) & (fcount > 0)
    kv = keep[lab]
    kf = keep[lab[f[:, 0]]] if len(f) else np.zeros(0, bool)
    new = np.cumsum(kv) - 1
    old = np.flatnonzero(kv).astype(np.int32)
    fo = new[f[kf]].astype(np.int32).reshape(-1, 3)
    no = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(-1, 3)[kv]
    return v[kv], fo, no, old


def cells(verts, origin, cell, grid):
    """[V, 3] cell coordinates: clamp(floor((p - origin) / cell), 0, g - 1) in float32, NaN -> 0"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    c = np.asarray(cell, dtype=np.float32).reshape(3)
    g = np.asarray(grid, dtype=np.int64).reshape(3)
    q = (v - o) / c
    fl = np.fmin(np.fmax(np.floor(q), np.float32(0)), (g - 1).astype(np.float32))
    return np.minimum(fl.astype(np.int64), g - 1)


def cluster(verts, faces, origin, cell, grid, normals=None):
    """-> (verts [K, 3] f32, faces [F', 3] int32, normals [K, 3] | None, flagged [K] bool) as mesh.simplify"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(v)
    f = _check_faces(faces, V)
    g = np.asarray(grid, dtype=np.int64).reshape(3)
    org = np.asarray(origin, dtype=np.float32).reshape(3).astype(np.float64)
    cl = np.asarray(cell, dtype=np.float32).reshape(3).astype(np.float64)
    cc = cells(v, origin, cell, grid)
    lin = (cc[:, 0] * g[1] + cc[:, 1]) * g[2] + cc[:, 2]
    occ = np.unique(lin)                                                         # clusters in linear cell order
    K = len(occ)
    cid = np.searchsorted(occ, lin)
    # faces: drop collapsed ones, keep the first of each unordered triple
    fc = cid[f] if len(f) else np.zeros((0, 3), np.int64)
    ok = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    idx = np.flatnonzero(ok)
    if len(idx):
        _, first = np.unique(np.sort(fc[idx], axis=1), axis=0, return_index=True)
        surv = np.sort(idx[first])
    else:
        surv = idx
    fo = fc[surv].astype(np.int32).reshape(-1, 3)
    # cluster corners (fp64, as the kernels)
    cz = occ % g[2]
    cy = (occ // g[2]) % g[1]
    cx = occ // g[2] // g[1]
    corner = org + cl * np.stack([cx, cy, cz], 1).astype(np.float64)               # [K, 3]
    acc = np.zeros((K, 16), dtype=np.int64)
    pv = v.astype(np.float64)
    u = (pv - corner[cid]) / cl
    np.add.at(acc[:, 9:12], cid, np.where(np.isnan(u), 0.0, np.rint(u * SP)).astype(np.int64))
    np.add.at(acc[:, 15], cid, 1)
    if normals is not None:
        n = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        np.add.at(acc[:, 12:15], cid, np.where(np.isnan(n), 0.0, np.rint(n * SN)).astype(np.int64))
    if len(f):
        p = pv[f]                                                                # [F, 3 verts, 3]
        e1 = (p[:, 1] - p[:, 0]) / cl
        e2 = (p[:, 2] - p[:, 0]) / cl
        m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        with np.errstate(invalid="ignore", over="ignore"):
            mm = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
            good = (mm > 0) & (mm < 1e300)
        m, mm, p, fcl = m[good], mm[good], p[good], fc[good]
        nrm = m / mm[:, None]
        area = 0.5 * mm
        an = [area * nrm[:, i] for i in range(3)]
        A = np.stack([an[0] * nrm[:, 0], an[0] * nrm[:, 1], an[0] * nrm[:, 2], an[1] * nrm[:, 1], an[1] * nrm[:, 2], an[2] * nrm[:, 2]], 1)
        qa = np.rint(A * SQ).astype(np.int64)
        for q in range(3):
            distinct = np.ones(len(fcl), bool)
            for r in range(q):
                distinct &= fcl[:, q] != fcl[:, r]
            c = fcl[distinct, q]
            o = corner[c]
            d = np.zeros(len(c))
            for a in range(3):
                d = d - nrm[distinct, a] * ((p[distinct, 0, a] - o[:, a]) / cl[a])
            np.add.at(acc[:, 0:6], c, qa[distinct])
            b = np.stack([np.rint(an[a][distinct] * d * SQ) for a in range(3)], 1).astype(np.int64)
            np.add.at(acc[:, 6:9], c, b)
    # representatives
    S = acc[:, 0:6].astype(np.float64) / SQ
    Am = np.stack([S[:, [0, 1, 2]], S[:, [1, 3, 4]], S[:, [2, 4, 5]]], 1)          # [K, 3, 3]
    b = acc[:, 6:9].astype(np.float64) / SQ
    cnt = acc[:, 15].astype(np.float64)
    xb = acc[:, 9:12].astype(np.float64) / SP / np.maximum(cnt, 1)[:, None]
    x = xb.copy()
    flagged = np.zeros(K, bool)
    if K:
        w, vec = np.linalg.eigh(Am)
        wmax = w.max(axis=1)
        r = -b - np.einsum("kij,kj->ki", Am, xb)
        pos = wmax > 0
        ratio = np.where(pos[:, None], w / np.where(pos, wmax, 1.0)[:, None], 0.0)
        kept = pos[:, None] & (w >= EIG_CUT * wmax[:, None])
        flagged = (pos[:, None] & (ratio >= EIG_CUT / 2) & (ratio <= EIG_CUT * 2)).any(axis=1)
        coef = np.where(kept, np.einsum("kje,kj->ke", vec, r) / np.where(kept, w, 1.0), 0.0)
        x = xb + np.einsum("kje,ke->kj", vec, coef)
    vo = (corner + np.clip(x, 0.0, 1.0) * cl).astype(np.float32)
    no = None
    if normals is not None:
        s = acc[:, 12:15].astype(np.float64) / SN
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        no = np.where(ln[:, None] > 0, s / np.where(ln > 0, ln, 1.0)[:, None], 0.0).astype(np.float32)
    return vo, fo, no, flagged


def default_grid(verts, cell, origin=None):
    """simplify()'s defaults: origin = the vertices' minimum, grid reaching the maximum's cell"""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    c = np.asarray(cell if np.ndim(cell) else (cell, cell, cell), dtype=np.float32).reshape(3)
    o = v.min(axis=0) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    top = np.floor((v.max(axis=0) - o) / c)
    return o, c, tuple(int(max(t, 0)) + 1 for t in top)
