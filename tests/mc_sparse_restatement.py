"""NumPy restatement of brick-sparse extraction: the selection of customnerf_amd.mesh.sparse_volume (probe lattice -> seed bricks -> growth)
and the marching cubes of csrc/mesh_sparse.hip over a brick list, on the table and in the float32 order of mc_restatement.  Test
infrastructure only.

A lattice point (x, y, z) lives in brick (x >> 3, y >> 3, z >> 3) at local index ((x & 7) * 8 + (y & 7)) * 8 + (z & 7); coords are sorted
lexicographically; nbr[b][(dx + 1) * 9 + (dy + 1) * 3 + dz + 1] is the brick at that offset or -1.  A point past the lattice's end does not
exist; a point inside it whose brick is not in the list is unavailable.  Everything works on `tiles`: every brick with one point below and
two above on each axis (local -1 .. 9), gathered through nbr.
"""
import numpy as np

import mc_restatement as R

B = 8
OFF = np.array([[o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1] for o in range(27)], dtype=np.int64)


def brick_grid(shape):
    return tuple(-(-int(s) // B) for s in shape)


def build_nbr(coords, shape):
    gb = brick_grid(shape)
    lut = {tuple(int(x) for x in c): i for i, c in enumerate(coords)}
    nbr = np.full((len(coords), 27), -1, dtype=np.int32)
    for i, c in enumerate(coords):
        for s, o in enumerate(OFF):
            q = (int(c[0] + o[0]), int(c[1] + o[1]), int(c[2] + o[2]))
            if all(0 <= q[a] < gb[a] for a in range(3)):
                nbr[i, s] = lut.get(q, -1)
    return nbr


def gather(vol, coords):
    """values [n, 512] of the bricks from a dense volume (entries past the lattice's end: the clamped point's, never read)"""
    loc = np.arange(B)
    out = np.empty((len(coords), B, B, B), dtype=np.float32)
    for i, c in enumerate(coords):
        ix = [np.minimum(int(c[a]) * B + loc, vol.shape[a] - 1) for a in range(3)]
        out[i] = vol[np.ix_(*ix)]
    return out.reshape(len(coords), B ** 3)


_RNG = {-1: (slice(0, 1), slice(7, 8)), 0: (slice(1, 9), slice(0, 8)), 1: (slice(9, 11), slice(0, 2))}   # offset -> (tile, local) range


def tiles(values, coords, nbr, shape):
    """-> T [n, 11, 11, 11] values at local -1 .. 9 (0 where there is none), A the point's brick is in the list, E the point exists"""
    n = len(coords)
    V = np.asarray(values, dtype=np.float32).reshape(n, B, B, B)
    T = np.zeros((n, 11, 11, 11), dtype=np.float32)
    A = np.zeros((n, 11, 11, 11), dtype=bool)
    for s, (dx, dy, dz) in enumerate(OFF):
        idx = np.flatnonzero(nbr[:, s] >= 0)
        if not len(idx):
            continue
        (tx, lx), (ty, ly), (tz, lz) = _RNG[int(dx)], _RNG[int(dy)], _RNG[int(dz)]
        T[idx, tx, ty, tz] = V[nbr[idx, s]][:, lx, ly, lz]
        A[idx, tx, ty, tz] = True
    g = [np.asarray(coords)[:, a, None].astype(np.int64) * B + np.arange(-1, 10)[None] for a in range(3)]
    e = [(g[a] >= 0) & (g[a] < shape[a]) for a in range(3)]
    E = e[0][:, :, None, None] & e[1][:, None, :, None] & e[2][:, None, None, :]
    return T, A, E


def _sh(X, d):
    """X at the bricks' own points shifted by d"""
    return X[:, 1 + d[0]:9 + d[0], 1 + d[1]:9 + d[1], 1 + d[2]:9 + d[2]]


def _classify(values, coords, nbr, shape, level):
    """-> T, mask [n, 8, 8, 8], case [n, 8, 8, 8] (both before the completeness rule), crosses [n], complete [n]"""
    T, A, E = tiles(values, coords, nbr, shape)
    inside = T >= np.float32(level)
    ex, in0 = _sh(E, (0, 0, 0)), _sh(inside, (0, 0, 0))
    mask = np.zeros(ex.shape, dtype=np.int64)
    h = []
    for a in range(3):
        d = tuple(int(a == b) for b in range(3))
        h.append(ex & _sh(E, d))
        mask |= (h[a] & _sh(A, d) & (_sh(inside, d) != in0)).astype(np.int64) << a
    case = np.zeros(ex.shape, dtype=np.int64)
    avail = np.ones(ex.shape, dtype=bool)
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
        avail &= _sh(A, d)
        case |= _sh(inside, d).astype(np.int64) << k
    case = np.where(h[0] & h[1] & h[2] & avail, case, 0)
    crosses = ((mask != 0) | ((case != 0) & (case != 255))).reshape(len(coords), -1).any(1)
    gb = np.array(brick_grid(shape))
    c = np.asarray(coords)[:, None, :].astype(np.int64) + OFF[None]
    in_grid = ((c >= 0) & (c < gb)).all(-1)
    complete = (~in_grid | (nbr >= 0)).all(1)
    return T, mask, case, crosses, complete


def state(values, coords, nbr, shape, level):
    """uint8 [n]: bit 0 the brick crosses, bit 1 it is complete"""
    _, _, _, crosses, complete = _classify(values, coords, nbr, shape, level)
    return (crosses.astype(np.uint8) | (complete.astype(np.uint8) << 1))


def marching_cubes(values, coords, nbr, shape, level, spacing=(1, 1, 1), origin=(0, 0, 0), normals=True):
    """-> dict: verts [V, 3] f32, faces [F, 3] int32, normals [V, 3] f32 | None, keys [V] int64, open (bricks that cross and are not
    complete; verts and faces are those of the complete bricks)"""
    n = len(coords)
    coords = np.asarray(coords).astype(np.int64).reshape(n, 3)
    level = np.float32(level)
    sp, org = np.asarray(spacing, dtype=np.float32), np.asarray(origin, dtype=np.float32)
    T, mask, case, crosses, complete = _classify(values, coords, nbr, shape, level)
    mask = np.where(complete[:, None, None, None], mask, 0)
    case = np.where(complete[:, None, None, None], case, 0)
    nvert = np.array([bin(m).count("1") for m in range(8)])[mask.reshape(-1)]
    vbase = np.concatenate([[0], np.cumsum(nvert)[:-1]]) if n else np.zeros(0, np.int64)
    b, lx, ly, lz, ax = np.nonzero(((mask[..., None] >> np.arange(3)) & 1).astype(bool))    # (brick, local point, axis) order
    loc = np.stack([lx, ly, lz], 1)
    gi = coords[b] * B + loc                                                                # global lattice index [V, 3]
    p = loc + 1                                                                             # tile coordinates
    q = p + np.eye(3, dtype=np.int64)[ax]
    at = lambda c: T[b, c[:, 0], c[:, 1], c[:, 2]]                                          # noqa: E731
    with np.errstate(all="ignore"):
        t = (level - at(p)) / (at(q) - at(p))
        t = np.where(np.isnan(t), np.float32(0.5), np.minimum(np.maximum(t, np.float32(0)), np.float32(1))).astype(np.float32)
        fi = gi.astype(np.float32)
        verts = np.empty((len(b), 3), dtype=np.float32)
        for k in range(3):
            verts[:, k] = np.where(ax == k, org[k] + (fi[:, k] + t) * sp[k], org[k] + fi[:, k] * sp[k])
        nrm = None
        if normals:
            def grad(c, g):
                out = np.empty((len(b), 3), dtype=np.float32)
                for k in range(3):
                    e = np.eye(3, dtype=np.int64)[k]
                    lo, hi = g[:, k] > 0, g[:, k] + 1 < shape[k]
                    vp, vm = np.where(hi, at(c + e), at(c)), np.where(lo, at(c - e), at(c))
                    out[:, k] = (vp - vm) / (np.where(lo & hi, np.float32(2), np.float32(1)) * sp[k])
                return out
            g0, g1 = grad(p, gi), grad(q, gi + np.eye(3, dtype=np.int64)[ax])
            nv = -(g0 + t[:, None] * (g1 - g0))
            ln = np.sqrt(nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2])
            nrm = (nv / np.where(ln > 0, ln, np.float32(1)).astype(np.float32)[:, None]).astype(np.float32)
    keys = ((gi[:, 0] * shape[1] + gi[:, 1]) * shape[2] + gi[:, 2]) * 3 + ax
    # faces: (brick, local cell, table order); the owner of a table edge through nbr when it lies in a forward brick
    cflat, mflat = case.reshape(-1), mask.reshape(-1)
    cells = np.flatnonzero(R.NTRI[cflat] > 0)
    cc = cflat[cells]
    tris = R.TRI[cc][:, :15].reshape(-1, 5, 3)
    e = tris[np.arange(5)[None, :] < R.NTRI[cc][:, None]].astype(np.int64).reshape(-1, 3)
    cell_of = np.repeat(cells, R.NTRI[cc])
    cb, cl = cell_of // 512, cell_of % 512
    corner, axis = R.EDGE_CORNER[e], R.EDGE_AXIS[e]
    o = [(cl >> 6)[:, None] + (corner & 1), ((cl >> 3) & 7)[:, None] + ((corner >> 1) & 1), (cl & 7)[:, None] + ((corner >> 2) & 1)]
    slot = ((o[0] >> 3) + 1) * 9 + ((o[1] >> 3) + 1) * 3 + (o[2] >> 3) + 1
    ob = np.asarray(nbr)[cb[:, None], slot].astype(np.int64)
    assert (ob >= 0).all() or int((crosses & ~complete).sum()) > 0
    owner = ob * 512 + ((o[0] & 7) * 8 + (o[1] & 7)) * 8 + (o[2] & 7)
    rank = np.array([[bin(m & ((1 << a) - 1)).count("1") for a in range(3)] for m in range(8)])
    owner = np.maximum(owner, 0)
    faces = (vbase[owner] + rank[mflat[owner], axis]).astype(np.int32).reshape(-1, 3)
    return dict(verts=verts, faces=faces, normals=nrm, keys=keys.astype(np.int64), open=int((crosses & ~complete).sum()))


def probe_index(n, probe):
    idx = list(range(0, n, probe))
    if idx[-1] != n - 1:
        idx.append(n - 1)
    return np.array(idx)


def seeds(vol, level, probe):
    """sorted coords of the seed bricks: the probe values with index in [8 b - probe, 8 b + 8 + probe]^3 are not all on one side"""
    pidx = [probe_index(n, probe) for n in vol.shape]
    inside = vol[np.ix_(*pidx)] >= np.float32(level)
    gb = brick_grid(vol.shape)
    sel = [[np.flatnonzero((pidx[a] >= B * k - probe) & (pidx[a] <= B * k + B + probe)) for k in range(gb[a])] for a in range(3)]
    out = []
    for i in range(gb[0]):
        for j in range(gb[1]):
            for k in range(gb[2]):
                sub = inside[np.ix_(sel[0][i], sel[1][j], sel[2][k])]
                if sub.any() and not sub.all():
                    out.append((i, j, k))
    return np.array(out, dtype=np.int32).reshape(-1, 3), int(inside.size)


def select(vol, level, probe=1, max_rounds=64):
    """The selection of mesh.sparse_volume on a field given as its dense volume -> dict: coords, values, nbr, rounds, evaluations"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    coords, evaluations = seeds(vol, level, probe)
    have = {tuple(int(x) for x in c) for c in coords}
    gb = brick_grid(vol.shape)
    rounds = 0
    while True:
        coords = np.array(sorted(have), dtype=np.int32).reshape(-1, 3)
        values, nbr = gather(vol, coords), build_nbr(coords, vol.shape)
        if not len(coords):
            break
        if rounds >= max_rounds:
            raise ValueError("still growing")
        rounds += 1                                  # a round: one pass over the bricks' states; the last finds nothing missing
        st = state(values, coords, nbr, vol.shape, level)
        need = set()
        for c in coords[(st & 1).astype(bool)]:
            for o in OFF:
                q = (int(c[0] + o[0]), int(c[1] + o[1]), int(c[2] + o[2]))
                if all(0 <= q[a] < gb[a] for a in range(3)) and q not in have:
                    need.add(q)
        if not need:
            break
        have |= need
    evaluations += 512 * len(coords)
    return dict(coords=coords, values=values, nbr=nbr, rounds=rounds, evaluations=evaluations)


def reorder(verts, faces, normals, keys):
    """the mesh in the dense pass's order: vertices sorted by key, faces remapped and sorted lexicographically by row"""
    order = np.argsort(keys, kind="stable")
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order))
    f = inv[np.asarray(faces, dtype=np.int64)]
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))] if len(f) else f
    return verts[order], f, None if normals is None else normals[order]


def sorted_rows(faces):
    f = np.asarray(faces, dtype=np.int64)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))] if len(f) else f


def volumes():
    """[(name, volume, level, spacing, origin)] that the host and the GPU tests extract densely and sparsely"""
    out = []
    g = lambda shape: np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij")     # noqa: E731
    X, Y, Z = g((17, 9, 26))                                    # a partial last brick on every axis, a 3 x 2 x 4 brick grid
    out.append(("partial_bricks", (5.5 - np.sqrt((X - 8.2) ** 2 + (Y - 4.1) ** 2 * 2 + (Z - 12.7) ** 2 / 4)).astype(np.float32), 0.0,
                (0.5, 0.25, 1.5), (3.0, -2.0, 0.5)))
    X, Y, Z = g((5, 5, 5))                                      # one brick, smaller than a brick
    out.append(("one_brick", (1.6 - np.sqrt((X - 2.1) ** 2 + (Y - 1.9) ** 2 + (Z - 2.2) ** 2)).astype(np.float32), 0.0, (1, 1, 1), (0, 0, 0)))
    import mesh_testlib
    _, vol, sp, org = mesh_testlib.speckled_sphere(56)          # components of 1.4 - 2.7 steps in radius
    out.append(("speckled_sphere", vol, 0.0, sp, org))
    out.append(("random", np.random.default_rng(5).random((19, 23, 17), dtype=np.float32), 0.5, (1, 1, 1), (0, 0, 0)))
    X, Y, Z = g((24, 12, 12))
    out.append(("plane_7_5", (7.5 - X).astype(np.float32), 0.0, (1, 1, 1), (0, 0, 0)))       # crossings on a brick boundary
    out.append(("plane_8_0", (8.0 - X).astype(np.float32), 0.0, (1, 1, 1), (0, 0, 0)))       # exactly at level: the t = 0 clamp
    X, Y, Z = g((26, 26, 20))                                   # cut by the lattice's faces: one-sided gradients, open rims
    out.append(("cut_sphere", (11.0 - np.sqrt((X - 12.5) ** 2 + (Y - 12.5) ** 2 + (Z - 3.0) ** 2)).astype(np.float32), 0.0,
                (2.0 / 25, 2.0 / 25, 2.0 / 19), (-1.0, -1.0, -1.0)))
    X, Y, Z = g((20, 18, 21))
    vol = (6.3 - np.sqrt((X - 9.6) ** 2 + (Y - 8.7) ** 2 + (Z - 10.2) ** 2)).astype(np.float32)
    rng = np.random.default_rng(11)
    for v in (np.nan, np.inf, -np.inf):
        vol.reshape(-1)[rng.choice(vol.size, 60, replace=False)] = v
    out.append(("nonfinite", vol, 0.0, (1, 1, 1), (0, 0, 0)))
    return out
