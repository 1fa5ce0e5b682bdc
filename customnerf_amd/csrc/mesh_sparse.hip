// Marching cubes over a brick-sparse float32 volume (cnerf_marching_cubes_sparse_*): the passes of mesh.hip — count -> scan -> emit vertices
// -> emit faces, on the caller's stream, no atomics, no host synchronisation — over a sorted list of n bricks of 8^3 lattice points in
// place of every point of the lattice.  Arithmetic: mesh_mc.h, shared with mesh.hip term for term, so a surface that the bricks cover
// comes out with the dense pass's bits.  The NumPy restatement the tests pin it to: tests/mc_sparse_restatement.py.
//
// Lattice point (x, y, z) lives in brick (x >> 3, y >> 3, z >> 3) at local index ((x & 7) 8 + (y & 7)) 8 + (z & 7); its flat index is
// brick * 512 + local, one thread each, and a workgroup of MC_BLOCK = 256 threads is half a brick (local x in 0..3 or 4..7).  nbr [n][27]
// names the bricks around a brick (-1: not in the list).  A point past the lattice's end does not exist (where the dense kernel's
// hx / hy / hz are false); a point inside the lattice whose brick is not in the list is unavailable.
//
//   k_mcs_count : stages the half-brick and one point beyond it on the upper side into LDS through nbr (resolved once per workgroup);
//                 case and edge mask of every point of a COMPLETE brick (all neighbour bricks inside the lattice present), 0 elsewhere;
//                 workgroup totals; one byte per workgroup: bit 0 some owned edge with both ends available changes side or some owned
//                 cell with 8 available corners is mixed, bit 1 the brick is complete
//   k_mcs_scan  : one workgroup: the scan of the totals, counts[3] = (vertices, triangles, open bricks = crossing and not complete),
//                 the optional state byte of every brick
//   k_mcs_verts : stages the half-brick with one point below and two above (the gradient of an edge's far end reaches that far);
//                 vertex bases, positions, normals, keys
//   k_mcs_faces : table edge -> owner point, through nbr when it lies in one of the 7 forward bricks
//
// Staging won against resolving nbr and reading global memory at every use (docs/HISTORY.md B.25 has the measurement).
// Workspace: the dense regions over n * 512 points | one byte per workgroup [2 n].
#include "mesh_mc.h"

#define MCS_B 8                  // points per brick and axis
#define MCS_PTS 512              // points per brick = 2 MC_BLOCK
#define MCS_HALF 4               // local x planes per workgroup

namespace {

struct McsPtr {
    McPtr mc;
    uint8_t *wflag;                                  // per workgroup: bit 0 crosses, bit 1 its brick is complete
};

uint64_t mcs_carve(void *ws, uint64_t n_bricks, McsPtr &p) {
    MeshCarve c(ws);
    mc_take(c, n_bricks * MCS_PTS, p.mc);
    p.wflag = c.take<uint8_t>(2 * n_bricks);
    return c.total();
}

struct McsVol {
    const float *__restrict__ values;
    const int32_t *__restrict__ coords, *__restrict__ nbr;
    uint32_t n_bricks, len[3];
};

// What a workgroup knows of its brick: the validated neighbour table in LDS, the brick's lattice origin, whether it is complete.
struct McsBrick {
    int32_t *nb;                                     // LDS [27]: brick index, or -1 (absent, or an index outside the list)
    int32_t org[3];                                  // global index of local (0, 0, 0); a brick outside the lattice gets len (nothing exists)
    uint32_t brick, half;
    bool complete;
};

// every thread of the block must call it; ends with a barrier
__device__ __forceinline__ void mcs_brick(const McsVol &v, int32_t *nb_lds, McsBrick &b) {
    b.nb = nb_lds;
    b.brick = blockIdx.x >> 1;
    b.half = blockIdx.x & 1u;
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int32_t c = v.coords[3 * (uint64_t)b.brick + a];
        const int32_t gb = (int32_t)((v.len[a] + MCS_B - 1) / MCS_B);
        bad |= c < 0 || c >= gb;
        b.org[a] = c * MCS_B;
    }
    if (bad) {
#pragma unroll
        for (int a = 0; a < 3; ++a) b.org[a] = (int32_t)v.len[a];
    }
    int ok = 1;
    if (threadIdx.x < 27) {
        const int32_t k = v.nbr[27 * (uint64_t)b.brick + threadIdx.x];
        const int32_t r = (k >= 0 && (uint32_t)k < v.n_bricks) ? k : -1;
        nb_lds[threadIdx.x] = r;
        const int d[3] = {(int)threadIdx.x / 9 - 1, (int)(threadIdx.x / 3) % 3 - 1, (int)threadIdx.x % 3 - 1};
        bool inside = !bad;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int32_t o = b.org[a] + d[a] * MCS_B;
            inside &= o >= 0 && o < (int32_t)v.len[a];
        }
        ok = !inside || r >= 0;
    }
    b.complete = __syncthreads_and(ok) != 0;
}

// brick-local coordinate c in [-8, 15] -> neighbour slot offset in {-1, 0, 1}
__device__ __forceinline__ int mcs_boff(int c) { return ((c + MCS_B) >> 3) - 1; }

// index into nb[] of the brick that holds local (cx, cy, cz)
__device__ __forceinline__ int mcs_slot(int cx, int cy, int cz) { return (mcs_boff(cx) + 1) * 9 + (mcs_boff(cy) + 1) * 3 + mcs_boff(cz) + 1; }

__device__ __forceinline__ bool mcs_exists(const McsVol &v, const McsBrick &b, int cx, int cy, int cz) {
    const int32_t gx = b.org[0] + cx, gy = b.org[1] + cy, gz = b.org[2] + cz;
    return gx >= 0 && gy >= 0 && gz >= 0 && gx < (int32_t)v.len[0] && gy < (int32_t)v.len[1] && gz < (int32_t)v.len[2];
}

// flat index of the point at local (cx, cy, cz), coordinates in [-8, 15]; false when its brick is not there
__device__ __forceinline__ bool mcs_flat(const McsBrick &b, int cx, int cy, int cz, uint32_t &flat) {
    const int32_t k = b.nb[mcs_slot(cx, cy, cz)];
    flat = (uint32_t)k * MCS_PTS + (uint32_t)(((cx & 7) * MCS_B + (cy & 7)) * MCS_B + (cz & 7));
    return k >= 0;
}

// value at local (cx, cy, cz): 0 for a point that does not exist or is unavailable (never used by the arithmetic)
__device__ __forceinline__ float mcs_fetch(const McsVol &v, const McsBrick &b, int cx, int cy, int cz) {
    uint32_t flat;
    return (mcs_flat(b, cx, cy, cz, flat) && mcs_exists(v, b, cx, cy, cz)) ? v.values[flat] : 0.0f;
}

// The values a workgroup reads: its half-brick with LO points below and HI points above on every axis, copied into LDS once.
template <int LO, int HI>
struct McsTile {
    static constexpr int TX = MCS_HALF + LO + HI, TY = MCS_B + LO + HI, TZ = MCS_B + LO + HI, SIZE = TX * TY * TZ;
    float *lds;
    const McsVol &v;
    const McsBrick &b;
    int x0;                                          // local x of the tile's first plane
    __device__ McsTile(float *lds_, const McsVol &v_, const McsBrick &b_) : lds(lds_), v(v_), b(b_), x0((int)b_.half * MCS_HALF - LO) {}
    // every thread of the block must call it (`work`: block-uniform; a workgroup with nothing to do skips the copy)
    __device__ __forceinline__ void fill(bool work) {
        if (work) {
            for (int i = (int)threadIdx.x; i < SIZE; i += MC_BLOCK) {
                const int tz = i % TZ, r = i / TZ, ty = r % TY, tx = r / TY;
                lds[i] = mcs_fetch(v, b, x0 + tx, ty - LO, tz - LO);
            }
        }
        __syncthreads();
    }
    __device__ __forceinline__ float at(int cx, int cy, int cz) const {
        return lds[((cx - x0) * TY + (cy + LO)) * TZ + (cz + LO)];
    }
};

// this thread's point: local coordinates, flat index, global indices (valid when it exists)
struct McsPoint {
    int c[3];
    uint32_t flat;
};

__device__ __forceinline__ McsPoint mcs_point(const McsBrick &b) {
    McsPoint p;
    p.c[0] = (int)(b.half * MCS_HALF + (threadIdx.x >> 6));
    p.c[1] = (int)((threadIdx.x >> 3) & 7u);
    p.c[2] = (int)(threadIdx.x & 7u);
    p.flat = blockIdx.x * MC_BLOCK + threadIdx.x;
    return p;
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcs_count(McsVol v, float level, uint8_t *__restrict__ cases, uint8_t *__restrict__ masks,
                                                        uint2 *__restrict__ sums, uint8_t *__restrict__ wflag) {
    typedef McsTile<0, 1> Tile;
    __shared__ uint32_t red_v[MC_WAVES], red_t[MC_WAVES];
    __shared__ int32_t nb[27];
    __shared__ float lds[Tile::SIZE];
    McsBrick b;
    mcs_brick(v, nb, b);
    Tile tile(lds, v, b);
    tile.fill(true);
    const McsPoint p = mcs_point(b);
    uint32_t m = 0, c = 0, ntri = 0;
    int cross = 0;
    if (mcs_exists(v, b, p.c[0], p.c[1], p.c[2])) {
        const bool in0 = mc_in(tile.at(p.c[0], p.c[1], p.c[2]), level);
        bool h[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int q[3] = {p.c[0] + (a == 0), p.c[1] + (a == 1), p.c[2] + (a == 2)};
            h[a] = mcs_exists(v, b, q[0], q[1], q[2]);
            if (h[a] && nb[mcs_slot(q[0], q[1], q[2])] >= 0 && mc_in(tile.at(q[0], q[1], q[2]), level) != in0) m |= 1u << a;
        }
        if (h[0] && h[1] && h[2]) {
            bool avail = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int q[3] = {p.c[0] + (k & 1), p.c[1] + ((k >> 1) & 1), p.c[2] + ((k >> 2) & 1)};
                avail &= nb[mcs_slot(q[0], q[1], q[2])] >= 0;
                c |= (uint32_t)mc_in(tile.at(q[0], q[1], q[2]), level) << k;
            }
            if (!avail) c = 0;
        }
        cross = m != 0 || (c != 0 && c != 255u);
        if (!b.complete) m = c = 0;                  // only complete bricks are meshed
        ntri = cn_mc_ntri[c];
    }
    cases[p.flat] = (uint8_t)c;
    masks[p.flat] = (uint8_t)m;
    const uint32_t tv = mc_block_total<2>((uint32_t)__popc(m), red_v);
    const uint32_t tt = mc_block_total<3>(ntri, red_t);
    const int any = __syncthreads_or(cross);
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = make_uint2(tv, tt);
        wflag[blockIdx.x] = (uint8_t)((any ? 1u : 0u) | (b.complete ? 2u : 0u));
    }
}

// one workgroup; as k_mc_scan, plus the bricks' states and counts[2] = open bricks; flag[1] = 1 when there are any (emit writes nothing)
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_mcs_scan(uint2 *__restrict__ sums, uint32_t n_bricks, const uint8_t *__restrict__ wflag,
                                                            uint8_t *__restrict__ state, uint32_t *__restrict__ counts,
                                                            uint32_t *__restrict__ flag) {
    __shared__ uint32_t wopen[MC_SCAN_BLOCK / CN_WAVE];
    uint64_t cv, ct;
    mc_scan_totals(sums, 2 * n_bricks, cv, ct);
    uint32_t open = 0;
    for (uint32_t k = threadIdx.x; k < n_bricks; k += MC_SCAN_BLOCK) {
        const uint32_t f0 = wflag[2 * (uint64_t)k], f1 = wflag[2 * (uint64_t)k + 1];
        const uint32_t st = ((f0 | f1) & 1u) | (f0 & 2u);
        if (state) state[k] = (uint8_t)st;
        open += st == 1u;
    }
    const uint32_t tot = cn_wave_sum(open);
    if (cn_lane() == 0) wopen[threadIdx.x / CN_WAVE] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int j = 0; j < MC_SCAN_BLOCK / CN_WAVE; ++j) s += wopen[j];
        mc_store_counts(cv, ct, counts, flag);
        counts[2] = s;
        flag[1] = s ? 1u : 0u;
    }
}

// mc_grad's fetch: the value d steps along `axis` from local point c
template <class Tile>
struct McsVal {
    const Tile &tile;
    int c[3], axis;
    __device__ __forceinline__ float operator()(int d) const {
        return tile.at(c[0] + (axis == 0 ? d : 0), c[1] + (axis == 1 ? d : 0), c[2] + (axis == 2 ? d : 0));
    }
};

__global__ __launch_bounds__(MC_BLOCK) void k_mcs_verts(McsVol v, float level, McGeom g, const uint8_t *__restrict__ masks,
                                                        const uint2 *__restrict__ sums, const uint32_t *__restrict__ flag,
                                                        const uint8_t *__restrict__ wflag, uint32_t *__restrict__ vbase,
                                                        float *__restrict__ verts, float *__restrict__ normals,
                                                        long long *__restrict__ keys, uint32_t max_verts) {
    typedef McsTile<1, 2> Tile;
    __shared__ uint32_t red[MC_WAVES];
    __shared__ int32_t nb[27];
    __shared__ float lds[Tile::SIZE];
    if (flag[0] | flag[1]) return;                   // overflow, or open bricks: nothing is written
    McsBrick b;
    mcs_brick(v, nb, b);
    Tile tile(lds, v, b);
    tile.fill((wflag[blockIdx.x] & 3u) == 3u);       // an incomplete or non-crossing half has no vertex
    const McsPoint p = mcs_point(b);
    const uint32_t m = masks[p.flat];
    const uint32_t base = sums[blockIdx.x].x + mc_block_prefix<2>((uint32_t)__popc(m), red);
    vbase[p.flat] = base;
    if (!m) return;
    const uint32_t idx[3] = {(uint32_t)(b.org[0] + p.c[0]), (uint32_t)(b.org[1] + p.c[1]), (uint32_t)(b.org[2] + p.c[2])};
    const float v0 = tile.at(p.c[0], p.c[1], p.c[2]);
    uint32_t vid = base;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((m >> a) & 1u)) continue;
        if (vid < max_verts) {
            const int q[3] = {p.c[0] + (a == 0), p.c[1] + (a == 1), p.c[2] + (a == 2)};
            const float t = mc_cross_t(level, v0, tile.at(q[0], q[1], q[2]));
            float pos[3];
            mc_vertex_pos(g, idx, a, t, pos);
            const uint64_t o = 3 * (uint64_t)vid;
            verts[o] = pos[0];
            verts[o + 1] = pos[1];
            verts[o + 2] = pos[2];
            if (keys) keys[vid] = (long long)((((uint64_t)idx[0] * v.len[1] + idx[1]) * v.len[2] + idx[2]) * 3 + (uint64_t)a);
            if (normals) {
                float g0[3], g1[3], nv[3];
#pragma unroll
                for (int bx = 0; bx < 3; ++bx) {
                    const uint32_t jb = bx == a ? idx[bx] + 1 : idx[bx];
                    g0[bx] = mc_grad(McsVal<Tile>{tile, {p.c[0], p.c[1], p.c[2]}, bx}, idx[bx], v.len[bx], g.sp[bx]);
                    g1[bx] = mc_grad(McsVal<Tile>{tile, {q[0], q[1], q[2]}, bx}, jb, v.len[bx], g.sp[bx]);
                }
                mc_normal(g0, g1, t, nv);
                normals[o] = nv[0];
                normals[o + 1] = nv[1];
                normals[o + 2] = nv[2];
            }
        }
        ++vid;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mcs_faces(McsVol v, const uint8_t *__restrict__ cases, const uint8_t *__restrict__ masks,
                                                        const uint2 *__restrict__ sums, const uint32_t *__restrict__ flag,
                                                        const uint32_t *__restrict__ vbase, int32_t *__restrict__ faces, uint32_t max_faces) {
    __shared__ uint32_t red[MC_WAVES];
    __shared__ int32_t nb[27];
    if (flag[0] | flag[1]) return;
    McsBrick b;
    mcs_brick(v, nb, b);
    const McsPoint p = mcs_point(b);
    const uint32_t c = cases[p.flat];
    const uint32_t nt = cn_mc_ntri[c];               // 0 outside complete bricks and for the points that own no cell
    const uint32_t base = sums[blockIdx.x].y + mc_block_prefix<3>(nt, red);
    for (uint32_t k = 0; k < nt; ++k) {
        const uint32_t f = base + k;
        if (f >= max_faces) break;
        int32_t tri[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            uint32_t corner, axis, owner;
            mc_edge_owner((uint32_t)cn_mc_tri[c][3 * k + q], corner, axis);
            // a crossing edge of a complete brick's cell has its owner in a brick of the list (else that brick were open)
            const bool there = mcs_flat(b, p.c[0] + (int)(corner & 1u), p.c[1] + (int)((corner >> 1) & 1u), p.c[2] + (int)((corner >> 2) & 1u), owner);
            tri[q] = there ? mc_vertex_id(vbase[owner], masks[owner], axis) : 0;
        }
        const uint64_t o = 3 * (uint64_t)f;
        faces[o] = tri[0];
        faces[o + 1] = tri[1];
        faces[o + 2] = tri[2];
    }
}

int mcs_check(uint32_t n_bricks, uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint32_t lim = 1u << 20;
    if (nx < 2 || ny < 2 || nz < 2 || nx > lim || ny > lim || nz > lim) return CNERF_EINVAL;
    if (n_bricks >= (1u << 22)) return CNERF_EINVAL;                          // the flat point index stays below 2^31
    return CNERF_OK;
}

}  // namespace

extern "C" {

int cnerf_marching_cubes_sparse_workspace_bytes(uint32_t n_bricks, uint64_t *bytes_host) {
    if (n_bricks >= (1u << 22)) return CNERF_EINVAL;
    if (!bytes_host) return CNERF_ENULL;
    McsPtr p;
    *bytes_host = mcs_carve(nullptr, n_bricks, p);
    return CNERF_OK;
}

int cnerf_marching_cubes_sparse_count(const float *values, const int32_t *coords, const int32_t *nbr, uint32_t n_bricks, uint32_t nx,
                                      uint32_t ny, uint32_t nz, float level, void *ws, uint64_t ws_bytes, uint8_t *state, uint32_t *counts,
                                      void *stream) {
    if (n_bricks == 0) return CNERF_OK;
    if (!values || !coords || !nbr || !ws || !counts) return CNERF_ENULL;
    if (const int rc = mcs_check(n_bricks, nx, ny, nz)) return rc;
    McsPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, mcs_carve(ws, n_bricks, p))) return rc;
    const McsVol v = {values, coords, nbr, n_bricks, {nx, ny, nz}};
    const dim3 grid(2 * n_bricks);
    hipLaunchKernelGGL(k_mcs_count, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), v, level, p.mc.cases, p.mc.masks, p.mc.sums, p.wflag);
    hipLaunchKernelGGL(k_mcs_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, CN_STREAM(stream), p.mc.sums, n_bricks, (const uint8_t *)p.wflag, state,
                       counts, p.mc.flag);
    return cn_launch_status();
}

int cnerf_marching_cubes_sparse_emit(const float *values, const int32_t *coords, const int32_t *nbr, uint32_t n_bricks, uint32_t nx,
                                     uint32_t ny, uint32_t nz, float level, const float *origin_host, const float *spacing_host, void *ws,
                                     uint64_t ws_bytes, float *verts, float *normals, int32_t *faces, int64_t *vert_keys, uint32_t max_verts,
                                     uint32_t max_faces, void *stream) {
    if (n_bricks == 0) return CNERF_OK;
    if (!values || !coords || !nbr || !origin_host || !spacing_host || !ws || (max_verts && !verts) || (max_faces && !faces)) return CNERF_ENULL;
    if (const int rc = mcs_check(n_bricks, nx, ny, nz)) return rc;
    McsPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, mcs_carve(ws, n_bricks, p))) return rc;
    const McsVol v = {values, coords, nbr, n_bricks, {nx, ny, nz}};
    const McGeom g = mc_geom(origin_host, spacing_host);
    const dim3 grid(2 * n_bricks);
    float *nrm = max_verts ? normals : nullptr;
    long long *keys = max_verts ? (long long *)vert_keys : nullptr;
    hipLaunchKernelGGL(k_mcs_verts, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), v, level, g, (const uint8_t *)p.mc.masks,
                       (const uint2 *)p.mc.sums, (const uint32_t *)p.mc.flag, (const uint8_t *)p.wflag, p.mc.vbase, verts, nrm, keys, max_verts);
    hipLaunchKernelGGL(k_mcs_faces, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), v, (const uint8_t *)p.mc.cases, (const uint8_t *)p.mc.masks,
                       (const uint2 *)p.mc.sums, (const uint32_t *)p.mc.flag, (const uint32_t *)p.mc.vbase, faces, max_faces);
    return cn_launch_status();
}

}  // extern "C"
