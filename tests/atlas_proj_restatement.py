"""NumPy restatement of the chart-based texture atlas (csrc/mesh_charts.hip, cnerf_mesh_atlas_proj_*), written from the rules in
include/customnerf_hip.h: classes in float32 with one rounding per operation, charts by union-find with the smallest node as root, extents
through the ordered integer image of the floats, the packing and the UVs in float64, ownership in int64.  Classes, charts, extents, the
density, rectangles, UVs, owner maps, totals and points are bit-equal to the device's."""
import numpy as np

import atlas_restatement as A

f32 = np.float32


class Plan:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _axis(c):
    """(k, s): the axis of the largest |c_k| (ties to the lowest k) and whether that component is negative; c [N, 3]"""
    a = np.abs(c)
    k = np.zeros(len(c), np.int64)
    k[a[:, 1] > a[:, 0]] = 1
    k[a[:, 2] > a[np.arange(len(c)), k]] = 2
    return k, c[np.arange(len(c)), k] < 0


def bad_index(v, f):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    return bool(((f < 0) | (f >= len(v))).any())


def classes(v, f, normals=None):
    """[F] int64: 2 k + (c_k < 0), or 6"""
    v = np.asarray(v, f32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    F = len(f)
    if not F:
        return np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
        q = ((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(f32)
        ok = (q > 0) & (q < np.inf)
        k, s = _axis(c)
        cls = 2 * k + s
        if normals is not None:
            n = np.asarray(normals, f32).reshape(-1, 3)
            g = ((n[f[:, 0]] + n[f[:, 1]]) + n[f[:, 2]]).astype(f32)
            use = np.isfinite(g).all(1) & (g != 0).any(1)
            gk, gs = _axis(np.where(np.isfinite(g), g, f32(0)))
            ck = c[np.arange(F), gk]
            adopt = use & ((ck < 0) == gs) & (f32(4) * (ck * ck).astype(f32) >= q)
            cls = np.where(adopt, 2 * gk + gs, cls)
    return np.where(ok, cls, 6).astype(np.int64)


def charts(f, cls):
    """(face_chart [F] int64 (-1: none), C): components of the nodes 6 v + class, ranked by their smallest node"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in np.nonzero(cls < 6)[0]:
        nodes = [int(6 * f[i, q] + cls[i]) for q in range(3)]
        for x in nodes:
            parent.setdefault(x, x)
        for a, b in ((nodes[0], nodes[1]), (nodes[1], nodes[2])):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = sorted(x for x in parent if parent[x] == x)
    rank = {r: i for i, r in enumerate(roots)}
    fc = np.full(len(f), -1, np.int64)
    for i in np.nonzero(cls < 6)[0]:
        fc[i] = rank[find(int(6 * f[i, 0] + cls[i]))]
    return fc, len(roots)


def project(v, f, cls):
    """(a, b) float32 [F, 3] of the corners of every face (0 for class 6)"""
    v = np.asarray(v, f32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    k = np.where(cls < 6, cls // 2, 0)
    neg = (cls % 2 == 1) & (cls < 6)
    ia = np.where(neg, (k + 2) % 3, (k + 1) % 3)
    ib = np.where(neg, (k + 1) % 3, (k + 2) % 3)
    safe = np.where((cls < 6)[:, None], f, 0)
    p = v[safe] if len(v) else np.zeros((len(f), 3, 3), f32)                   # [F, 3 corners, 3]
    r = np.arange(len(f))[:, None]
    a, b = p[r, np.arange(3)[None], ia[:, None]], p[r, np.arange(3)[None], ib[:, None]]
    return a.astype(f32), b.astype(f32)


def _enc(x):
    u = np.asarray(x, f32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xffffffff, u | 0x80000000).astype(np.uint32)


def _dec(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32).view(f32)


def extents(a, b, fc, C):
    """float32 [C, 4] = (a0, a1, b0, b1): min / max on the ordered image, so that -0 lies below +0"""
    e = np.zeros((C, 4), np.uint32)
    e[:, 0] = e[:, 2] = 0xffffffff
    m = fc >= 0
    idx = np.repeat(fc[m], 3)
    ia, ib = _enc(a[m].reshape(-1)), _enc(b[m].reshape(-1))
    np.minimum.at(e[:, 0], idx, ia)
    np.maximum.at(e[:, 1], idx, ia)
    np.minimum.at(e[:, 2], idx, ib)
    np.maximum.at(e[:, 3], idx, ib)
    return _dec(e).reshape(C, 4)


def _sizes(ext, rho, g):
    e = np.asarray(ext, f32).reshape(-1, 4).astype(np.float64)
    w = np.ceil(rho * (e[:, 1] - e[:, 0])) + 1.0 + 2.0 * g
    h = np.ceil(rho * (e[:, 3] - e[:, 2])) + 1.0 + 2.0 * g
    return w, h


def shelves(ext, rho, R, g):
    """rects int64 [C, 4] = (X0, Y0, w, h) of the shelf packing at density rho, or None when it does not fit"""
    w, h = _sizes(ext, rho, g)
    C = len(w)
    if not (np.all(w <= R) and np.all(h <= R)):
        return None
    order = sorted(range(C), key=lambda c: (-h[c], -w[c], c))
    rects = np.zeros((C, 4), np.int64)
    x = y = 0
    H = int(h[order[0]]) if C else 0
    for c in order:
        wc, hc = int(w[c]), int(h[c])
        if x + wc > R:
            y += H
            x = 0
            H = hc
        if y + H > R:
            return None
        rects[c] = (x, y, wc, hc)
        x += wc
    return rects


def pack(ext, R, g):
    """(rho float64, rects int64 [C, 4]); ValueError when the charts do not fit at rho = 0 or an argument is out of range"""
    e = np.asarray(ext, f32).reshape(-1, 4).astype(np.float64)
    if R < 16 or R > 16384 or g < 0 or g > 8:
        raise ValueError("resolution or gutter")
    if not len(e):
        return 0.0, np.zeros((0, 4), np.int64)
    da, db = e[:, 1] - e[:, 0], e[:, 3] - e[:, 2]
    if not (np.all(da >= 0) and np.all(db >= 0) and np.all(np.isfinite(da)) and np.all(np.isfinite(db))):
        raise ValueError("extents")
    if shelves(ext, 0.0, R, g) is None:
        raise ValueError("the charts do not fit")
    D = max(da.max(), db.max())
    rho = 0.0
    hi = (float(R) - 1.0 - 2.0 * g) / D if D > 0 else 0.0
    if hi > 0 and np.isfinite(hi):
        if shelves(ext, hi, R, g) is not None:
            rho = hi
        else:
            lo = 0.0
            for _ in range(24):
                m = 0.5 * (lo + hi)
                if shelves(ext, m, R, g) is not None:
                    lo = m
                else:
                    hi = m
            rho = lo
    return float(rho), shelves(ext, rho, R, g)


def corners(a, b, fc, ext, rects, rho, R, g):
    """(tx, ty float64 [F, 3] in texel space, uvs float32 [F, 3, 2], snap int64 [F, 3, 2]); zeros for uncharted faces"""
    F = len(fc)
    m = fc >= 0
    c = np.where(m, fc, 0)
    tx, ty = np.zeros((F, 3)), np.zeros((F, 3))
    if F and len(rects):
        e = np.asarray(ext, f32).astype(np.float64)[c]
        rc = np.asarray(rects, np.int64)[c].astype(np.float64)
        ox = (rc[:, 0] + g) + 0.5
        oy = (rc[:, 1] + rc[:, 3] - 1 - g) + 0.5
        tx = ox[:, None] + rho * (a.astype(np.float64) - e[:, 0:1])
        ty = oy[:, None] - rho * (b.astype(np.float64) - e[:, 2:3])
    tx, ty = np.where(m[:, None], tx, 0.0), np.where(m[:, None], ty, 0.0)
    u, w = (tx / float(R)).astype(f32), (1.0 - ty / float(R)).astype(f32)
    uv = np.where(m[:, None, None], np.stack([u, w], -1), f32(0)).astype(f32)
    snap = np.stack([np.rint(256.0 * tx), np.rint(256.0 * ty)], -1).astype(np.int64)
    return tx, ty, uv, snap


def _edges(s, px, py):
    """A and (E_0, E_1, E_2) of the face with snapped corners s [3, 2] at the points (px, py)"""
    x, y = s[:, 0], s[:, 1]
    A = (y[1] - y[0]) * (x[2] - x[0]) - (x[1] - x[0]) * (y[2] - y[0])
    E = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        E.append((y[j] - y[i]) * (px - x[i]) - (x[j] - x[i]) * (py - y[i]))
    return A, E


def _area2(snap):
    x, y = snap[..., 0], snap[..., 1]
    return (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0]) - (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0])


def owners(snap, fc, R):
    """(owner map after pass A, after A and B: int64 [R, R], -1 none; overlap_texels)"""
    big = np.iinfo(np.int64).max
    ma = np.full((R, R), big, np.int64)
    charted = np.nonzero(fc >= 0)[0]
    A2 = _area2(snap) if len(snap) else np.zeros(0, np.int64)
    for f in charted:                                                          # pass A
        if A2[f] <= 0:
            continue
        s = snap[f]
        X0, X1 = max(0, -((128 - s[:, 0].min()) // 256)), min(R - 1, (s[:, 0].max() - 128) // 256)
        Y0, Y1 = max(0, -((128 - s[:, 1].min()) // 256)), min(R - 1, (s[:, 1].max() - 128) // 256)
        if X1 < X0 or Y1 < Y0:
            continue
        Y, X = np.meshgrid(np.arange(Y0, Y1 + 1), np.arange(X0, X1 + 1), indexing="ij")
        _, E = _edges(s, 256 * X + 128, 256 * Y + 128)
        inside = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
        sub = ma[Y0:Y1 + 1, X0:X1 + 1]
        sub[inside] = np.minimum(sub[inside], f)
    mb = np.full((R, R), big, np.int64)
    overlap = 0
    for f in charted:                                                          # pass B and the overlap count
        s = snap[f]
        X0, X1 = max(0, -((256 - s[:, 0].min()) // 256)), min(R - 1, s[:, 0].max() // 256)
        Y0, Y1 = max(0, -((256 - s[:, 1].min()) // 256)), min(R - 1, s[:, 1].max() // 256)
        if X1 < X0 or Y1 < Y0:
            continue
        Y, X = np.meshgrid(np.arange(Y0, Y1 + 1), np.arange(X0, X1 + 1), indexing="ij")
        A, E = _edges(s, 256 * X + 128, 256 * Y + 128)
        claim = np.ones(X.shape, bool)
        if A > 0:
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3
                claim &= E[k] + 128 * (abs(s[j, 0] - s[i, 0]) + abs(s[j, 1] - s[i, 1])) >= 0
            strict = (E[0] > 0) & (E[1] > 0) & (E[2] > 0)
            overlap += int((strict & (ma[Y0:Y1 + 1, X0:X1 + 1] != f)).sum())
        claim &= ma[Y0:Y1 + 1, X0:X1 + 1] == big
        sub = mb[Y0:Y1 + 1, X0:X1 + 1]
        sub[claim] = np.minimum(sub[claim], f)
    own_a = np.where(ma != big, ma, -1)
    own_ab = np.where(ma != big, ma, np.where(mb != big, mb, -1))
    return own_a, own_ab, overlap


def grow(owner, g):
    """g Jacobi rounds: W, E, N, S, NW, NE, SW, SE, N the row above"""
    o = owner.copy()
    R = len(o)
    for _ in range(g):
        pad = np.full((R + 2, R + 2), -1, np.int64)
        pad[1:-1, 1:-1] = o
        new = o.copy()
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)):
            nb = pad[1 + dy:R + 1 + dy, 1 + dx:R + 1 + dx]
            take = (new < 0) & (nb >= 0)
            new[take] = nb[take]
        o = new
    return o


def plan(v, f, R, normals=None, g=2):
    """every stage of the layout -> Plan"""
    v = np.asarray(v, f32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    assert not bad_index(v, f)
    cls = classes(v, f, normals)
    fc, C = charts(f, cls)
    a, b = project(v, f, cls)
    ext = extents(a, b, fc, C)
    rho, rects = pack(ext, R, g)
    tx, ty, uv, snap = corners(a, b, fc, ext, rects, rho, R, g)
    own_a, own_ab, overlap = owners(snap, fc, R)
    own = grow(own_ab, g)
    Y, X = np.nonzero(own >= 0)                                                # row-major
    return Plan(R=R, g=g, classes=cls, face_chart=fc, C=C, extents=ext, rho=rho, rects=rects, tx=tx, ty=ty, uvs=uv, snap=snap,
                owner_a=own_a, owner_ab=own_ab, owner=own, overlap=overlap, X=X, Y=Y, total=len(X))


def points(p, v, f, normals=None, t0=0, t1=None):
    """(x, d) float32 [N, 3] of the listed texels t in [t0, t1)"""
    v = np.asarray(v, f32).reshape(-1, 3)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    t1 = p.total if t1 is None else t1
    X, Y = p.X[t0:t1], p.Y[t0:t1]
    N = len(X)
    if not N:
        return np.zeros((0, 3), f32), np.zeros((0, 3), f32)
    fo = p.owner[Y, X]
    s = p.snap[fo]                                                             # [N, 3, 2]
    x, y = s[..., 0], s[..., 1]
    px, py = 256 * X + 128, 256 * Y + 128
    A2 = _area2(s)
    E = {}
    for k in (1, 2):
        i, j = (k + 1) % 3, (k + 2) % 3
        E[k] = (y[:, j] - y[:, i]) * (px - x[:, i]) - (x[:, j] - x[:, i]) * (py - y[:, i])
    pos = A2 > 0
    Ad = np.where(pos, A2, 1).astype(np.float64)
    w1 = np.where(pos, (E[1].astype(np.float64) / Ad).astype(f32), f32(0)).astype(f32)
    w2 = np.where(pos, (E[2].astype(np.float64) / Ad).astype(f32), f32(0)).astype(f32)
    tri = f[fo]
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    none = np.full(N, -1)
    with np.errstate(all="ignore"):
        xo = np.where(pos[:, None], A._interp(p0, p1, p2, w1, w2, none), p0).astype(f32)
        ok = np.zeros(N, bool)
        dd = np.zeros((N, 3), f32)
        if normals is not None:
            nv = np.asarray(normals, f32).reshape(-1, 3)
            dd, ok = A._look(A._interp(nv[tri[:, 0]], nv[tri[:, 1]], nv[tri[:, 2]], w1, w2, none))
        e1, e2 = p1 - p0, p2 - p0
        gn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(f32)
        dg, okg = A._look(gn)
        d = np.where(ok[:, None], dd, np.where(okg[:, None], dg, np.array([0, 0, -1], f32)))
    return xo, d.astype(f32)
