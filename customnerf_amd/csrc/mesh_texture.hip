// Texture atlas of a triangle mesh and texture baking (cnerf_mesh_atlas_*): a fixed per-face-pair layout, so that the owner of every texel
// follows from its index (no chart search, no packing state).  Same conventions as the other mesh passes: the caller's stream and buffers,
// no allocation, no host synchronisation, no float atomics (the output is bit-reproducible).  The rules are in include/customnerf_hip.h;
// the NumPy restatement the tests pin them to: tests/atlas_restatement.py.
//
//   k_atlas_uvs             : one thread per face corner: its UV (the centre of a corner texel) and the index check into flags bit 0
//   k_bake_points<AtlasGeom> : one thread per cell texel t in [t0, t1): its face, the surface point at its (unclamped) barycentrics and the
//                    view direction looking at the surface; the field is evaluated on these between this pass and the next
//   k_bake_store<AtlasGeom>  : one thread per cell texel: round(clamp(rgb, 0, 1) * 255) at its global position, the fill colour on an
//                    un-owned texel
//   k_bake_fill<AtlasGeom>   : one thread per image texel: the fill colour on every texel outside the first P cells (the others are the
//                    store pass's)
// The three k_bake_* kernels are mesh_bake.h's, shared by every layout; a layout says where a cell texel lies (AtlasGeom; SizedTexels,
// SizedCells).
// (They were k_atlas_points / _store / _fill, k_sized_points / _store / _fill and k_pj_points / _store / _fill, one copy per layout.)
//
// Every texel is independent: the passes are bound by their stores (24 B of points and directions per texel, 3 B of image per texel).
//
// The area-proportional layout (cnerf_mesh_atlas_sized_*; restatement: tests/atlas_sized_restatement.py) gives a face a cell of 4 * 2^k texels,
// k from its longest edge, and lays the cells along a Z-order curve, largest first.  Inside a cell every rule above holds with the cell's s:
//   k_sized_measure : one thread per face: its size key and the index check; the 2048-bin key histogram in LDS, flushed by integer atomics
//   k_sized_count / k_sized_scan / k_sized_emit : class and in-class rank (face order: the scans of mesh_common.h) -> the face's cell record
//                     (X0, Y0, s, b) and the cell -> (face A, face B) table
//   k_sized_uvs, k_bake_points / _store<SizedTexels>, k_bake_fill<SizedCells> : as the four above, reading the plan; a texel finds its class from the
//                     at most eight class offsets
#include "mesh_bake.h"

#define AT_BLOCK BK_BLOCK
#define AT_BAD_INDEX 1u

namespace {

// A cell texel of either layout: image texel e, owning face f (-1: none), local texel (i, j) in a cell of edge s.  Face A of the cell owns
// the texels up to the anti-diagonal, face B the ones beyond it.
struct CellTexel {
    uint32_t e;
    int32_t f;
    uint32_t i, j, s;
};

__device__ __forceinline__ uint32_t at_side(uint32_t i, uint32_t j, uint32_t s) { return i + j > s - 1 ? 1u : 0u; }

// the weights of a cell texel in its face, and the corner whose texel it is
__device__ __forceinline__ bool at_cell_bary(const CellTexel &tx, float &w1, float &w2, int &corner) {
    const uint32_t i = tx.i, j = tx.j, s = tx.s;
    if (!at_side(i, j, s)) {
        const float den = (float)(s - 2);
        w1 = (float)j / den;
        w2 = (float)i / den;
        corner = (i == 0 && j == 0) ? 0 : (i == 0 && j == s - 2) ? 1 : (i == s - 2 && j == 0) ? 2 : -1;
    } else {
        const float den = (float)(s - 3);
        w1 = (float)(s - 1 - j) / den;
        w2 = (float)(s - 1 - i) / den;
        corner = (i == s - 1 && j == s - 1) ? 0 : (i == s - 1 && j == 2) ? 1 : (i == 2 && j == s - 1) ? 2 : -1;
    }
    return true;
}

// The uniform layout, and its locator (mesh_bake.h): cell p = t / s^2 holds the faces 2 p and 2 p + 1
struct AtlasGeom {
    uint32_t F, R, n, s, P;
    typedef CellTexel Texel;
    static constexpr bool FILL_FLAGS = false;

    template <bool FACE>
    __device__ __forceinline__ bool find(uint32_t t, CellTexel &tx) const {
        const uint32_t s2 = s * s, p = t / s2, r = t - p * s2, j = r / s, i = r - j * s;
        const uint32_t f = 2 * p + at_side(i, j, s), cy = p / n, cx = p - cy * n;
        tx = {(cy * s + j) * R + cx * s + i, f < F ? (int32_t)f : -1, i, j, s};
        return true;
    }
    __device__ __forceinline__ bool bary(const CellTexel &tx, float &w1, float &w2, int &corner) const {
        return at_cell_bary(tx, w1, w2, corner);
    }
    __device__ __forceinline__ bool stored(uint32_t e) const {  // a used cell
        const uint32_t Y = e / R, X = e - Y * R, cx = X / s, cy = Y / s;
        return cx < n && cy < n && cy * n + cx < P;
    }
};

// host: the layout of F faces on an R x R image, or CNERF_EINVAL
int at_layout(uint32_t F, uint32_t R, AtlasGeom *g) {
    if (R < 16 || R > 16384 || F >= (1u << 31)) return CNERF_EINVAL;
    const uint32_t P = (uint32_t)(((uint64_t)F + 1) / 2);
    uint64_t n = 1;
    while (n * n < P) n = n < 2 ? 2 : n * 2;                  // power-of-two bracket, then bisection: ceil(sqrt(P)) exactly
    uint64_t lo = n / 2, hi = n;                             // lo^2 < P <= hi^2 (or P <= 1 and n = 1)
    while (hi - lo > 1) {
        const uint64_t m = (lo + hi) / 2;
        (m * m < P ? lo : hi) = m;
    }
    n = P <= 1 ? 1 : hi;
    const uint64_t s = R / n;
    if (s < 4) return CNERF_EINVAL;
    g->F = F;
    g->R = R;
    g->n = (uint32_t)n;
    g->s = (uint32_t)s;
    g->P = P;
    return CNERF_OK;
}

// local texel (i, j) of corner k of face A (b = 0) or B (b = 1) of a cell of edge s
__device__ __forceinline__ void at_corner(uint32_t b, uint32_t k, uint32_t s, uint32_t &i, uint32_t &j) {
    if (!b) {
        i = k == 2 ? s - 2 : 0u;
        j = k == 1 ? s - 2 : 0u;
    } else {
        i = k == 2 ? 2u : s - 1;
        j = k == 1 ? 2u : s - 1;
    }
}

// the UV of the centre of image texel (X, Y): v points up
__device__ __forceinline__ void at_uv(uint32_t X, uint32_t Y, uint32_t R, float *__restrict__ uv) {
    uv[0] = ((float)X + 0.5f) / (float)R;
    uv[1] = 1.0f - ((float)Y + 0.5f) / (float)R;
}

__global__ __launch_bounds__(AT_BLOCK) void k_atlas_uvs(const int32_t *__restrict__ faces, uint32_t V, AtlasGeom g, float *__restrict__ uvs,
                                                        uint32_t max_faces, uint32_t *__restrict__ flags) {
    const uint32_t c = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (c >= 3 * g.F) return;
    const int32_t v = faces[c];
    if (v < 0 || (uint32_t)v >= V) atomicOr(flags, AT_BAD_INDEX);
    const uint32_t f = c / 3, k = c - 3 * f;
    if (f >= max_faces) return;
    const uint32_t p = f >> 1, cy = p / g.n, cx = p - cy * g.n;
    uint32_t i, j;
    at_corner(f & 1u, k, g.s, i, j);
    at_uv(cx * g.s + i, cy * g.s + j, g.R, uvs + 2 * (uint64_t)c);
}

// ------------------------------------------------------------------------------------------------ the area-proportional layout
#define SZ_BINS 2048
#define SZ_CLASSES 8
#define SZ_MAX_F (1u << 25)                                  // 2 (16384 / 4)^2: more faces fit no resolution

// What every pass after the host read is given by value.  Classes lie along the Z-order curve from K down to 0: class k starts at tile
// O[k] (cell texel 16 O[k]) and at cell B[k] of the cell -> faces table; both are 0 for the (empty) classes above K.
struct SizedPlan {
    uint32_t F, R, K, tiles;
    uint32_t n[SZ_CLASSES], O[SZ_CLASSES], B[SZ_CLASSES];
};

struct SizedPtr {
    uint32_t *hdr, *key, *sums;
    int32_t *owner;                                          // [cells][2]: face A, face B or -1
};

uint64_t sz_carve(void *ws, uint64_t F, SizedPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.key = c.take<uint32_t>(F);
    p.sums = c.take<uint32_t>(cn_div_up64(F, MC_BLOCK) * SZ_CLASSES);
    p.owner = c.take<int32_t>(2 * F);                        // ceil(n_k / 2) <= n_k cells per class
    return c.total();
}

int sz_log2(uint32_t R) {                                    // log2 of a power of two in [16, 16384], else -1
    for (int l = 4; l <= 14; ++l)
        if (R == (1u << l)) return l;
    return -1;
}

// host: tiles of the classes with n[] faces each
uint64_t sz_tiles(const uint32_t n[SZ_CLASSES]) {
    uint64_t t = 0;
    for (int k = 0; k < SZ_CLASSES; ++k) t += (((uint64_t)n[k] + 1) / 2) << (2 * k);
    return t;
}

// host: the plan of counts n[] on an R x R image, or CNERF_EINVAL (R, a class above K, a sum that is not F, more tiles than the image has)
int sz_plan(uint32_t F, uint32_t R, const uint32_t *n, SizedPlan *p) {
    const int l = sz_log2(R);
    if (l < 0 || F > SZ_MAX_F) return CNERF_EINVAL;
    p->F = F;
    p->R = R;
    p->K = (uint32_t)(l - 2 < 7 ? l - 2 : 7);
    uint64_t sum = 0;
    for (int k = 0; k < SZ_CLASSES; ++k) {
        if (n[k] > F || ((uint32_t)k > p->K && n[k])) return CNERF_EINVAL;
        p->n[k] = n[k];
        sum += n[k];
    }
    const uint64_t tiles = sz_tiles(n), cap = (uint64_t)(R / 4) * (R / 4);
    if (sum != F || tiles > cap) return CNERF_EINVAL;
    uint32_t o = 0, b = 0;
    for (int k = SZ_CLASSES - 1; k >= 0; --k) {
        p->O[k] = o;
        p->B[k] = b;
        const uint32_t c = (n[k] + 1) / 2;
        o += c << (2 * k);
        b += c;
    }
    p->tiles = o;
    return CNERF_OK;
}

// the even bits of o, packed: the x of Z-order index o (its y: the even bits of o >> 1)
__device__ __forceinline__ uint32_t sz_even_bits(uint32_t o) {
    o &= 0x55555555u;
    o = (o | (o >> 1)) & 0x33333333u;
    o = (o | (o >> 2)) & 0x0f0f0f0fu;
    o = (o | (o >> 4)) & 0x00ff00ffu;
    o = (o | (o >> 8)) & 0x0000ffffu;
    return o;
}

// the bits of x < 2^16 spread to the even positions
__device__ __forceinline__ uint32_t sz_spread_bits(uint32_t x) {
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

__device__ __forceinline__ uint32_t sz_class(uint32_t key, uint32_t e, uint32_t K) {
    if (key < e) return 0;
    const uint32_t k = (key - e) >> 4;
    return k < K ? k : K;
}

__global__ __launch_bounds__(MC_BLOCK) void k_sized_measure(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ faces,
                                                            uint32_t F, uint32_t *__restrict__ key, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[SZ_BINS];
    for (uint32_t i = threadIdx.x; i < SZ_BINS; i += MC_BLOCK) h[i] = 0;
    __syncthreads();
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f < F) {
        uint32_t t[3];
        if (!mesh_face(faces, f, V, t)) {
            atomicOr(hist + SZ_BINS, AT_BAD_INDEX);
            key[f] = 0;
        } else {
            float p[3][3];
#pragma unroll
            for (int q = 0; q < 3; ++q) at_load3(verts, t[q], p[q]);
            float L2 = 0.0f;
#pragma unroll
            for (int q = 0; q < 3; ++q) {                    // edges (0,1), (1,2), (2,0)
                const float *a = p[q], *b = p[(q + 1) % 3];
                const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
                const float l = (dx * dx + dy * dy) + dz * dz;
                L2 = q ? fmaxf(L2, l) : l;                   // a NaN is ignored beside a number
            }
            const uint32_t kf = (L2 > 0.0f && L2 < INFINITY) ? __float_as_uint(L2) >> 20 : 0u;
            key[f] = kf;
            atomicAdd(&h[kf], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SZ_BINS; i += MC_BLOCK)
        if (h[i]) atomicAdd(hist + i, h[i]);
}

// workgroup totals of the eight classes
__global__ __launch_bounds__(MC_BLOCK) void k_sized_count(SizedPlan pl, uint32_t e, SizedPtr p) {
    __shared__ uint32_t red[SZ_CLASSES][MC_WAVES];
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t tot[SZ_CLASSES];
    mc_block_class_rank<SZ_CLASSES>(f < pl.F ? sz_class(p.key[f], e, pl.K) : SZ_CLASSES, red, tot);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < SZ_CLASSES; ++k) p.sums[(uint64_t)blockIdx.x * SZ_CLASSES + k] = tot[k];
    }
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_sized_scan(uint32_t nblk, SizedPtr p) {
    uint64_t tot[SZ_CLASSES];
    mc_scan_totals_n<SZ_CLASSES>(p.sums, nblk, tot);         // each at most F < 2^32
}

__global__ __launch_bounds__(MC_BLOCK) void k_sized_emit(SizedPlan pl, uint32_t e, SizedPtr p, const uint32_t *__restrict__ flags,
                                                         int32_t *__restrict__ cells, uint32_t max_faces) {
    __shared__ uint32_t red[SZ_CLASSES][MC_WAVES];
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t k = f < pl.F ? sz_class(p.key[f], e, pl.K) : SZ_CLASSES;
    uint32_t tot[SZ_CLASSES];
    uint32_t r = mc_block_class_rank<SZ_CLASSES>(k, red, tot);
    if (f >= pl.F || flags[0]) return;                       // after a bad index nothing is written
    r += p.sums[(uint64_t)blockIdx.x * SZ_CLASSES + k];
    uint32_t nk = 0, Ok = 0, Bk = 0;
#pragma unroll
    for (int q = 0; q < SZ_CLASSES; ++q)
        if (k == (uint32_t)q) {
            nk = pl.n[q];
            Ok = pl.O[q];
            Bk = pl.B[q];
        }
    if (r >= nk) return;                                     // counts that are not this mesh's: no cell to give
    const uint32_t c = r >> 1, b = r & 1u, o = Ok + (c << (2 * k));
    p.owner[2 * (uint64_t)(Bk + c) + b] = (int32_t)f;
    if (f >= max_faces) return;
    int32_t *rec = cells + 4 * (uint64_t)f;
    rec[0] = (int32_t)(4 * sz_even_bits(o));
    rec[1] = (int32_t)(4 * sz_even_bits(o >> 1));
    rec[2] = (int32_t)(4u << k);
    rec[3] = (int32_t)b;
}

__global__ __launch_bounds__(AT_BLOCK) void k_sized_uvs(uint32_t F, uint32_t R, const int32_t *__restrict__ cells,
                                                        const uint32_t *__restrict__ flags, float *__restrict__ uvs) {
    const uint32_t c = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (c >= 3 * F || flags[0]) return;
    const uint32_t f = c / 3, k = c - 3 * f;
    const int32_t *rec = cells + 4 * (uint64_t)f;
    uint32_t i, j;
    at_corner((uint32_t)rec[3], k, (uint32_t)rec[2], i, j);
    at_uv((uint32_t)rec[0] + i, (uint32_t)rec[1] + j, R, uvs + 2 * (uint64_t)c);
}

// cell texel t < 16 tiles -> its cell (index into the cell -> faces table, tile offset o), the cell's edge s and the local texel (i, j)
__device__ __forceinline__ void sz_texel(const SizedPlan &pl, uint32_t t, uint32_t &cell, uint32_t &o, uint32_t &s, uint32_t &i, uint32_t &j) {
    const uint32_t tile = t >> 4;
    uint32_t k = 0, Ok = pl.O[0], Bk = pl.B[0];
#pragma unroll
    for (int q = 1; q < SZ_CLASSES; ++q)                     // O[] descends with k: the class is the first whose offset is not above the tile
        if (tile < pl.O[q - 1]) {
            k = (uint32_t)q;
            Ok = pl.O[q];
            Bk = pl.B[q];
        }
    const uint32_t rel = t - (Ok << 4), c = rel >> (4 + 2 * k), r = rel & ((16u << (2 * k)) - 1);
    s = 4u << k;
    j = r >> (2 + k);
    i = r & (s - 1);
    cell = Bk + c;
    o = Ok + (c << (2 * k));
}

// The area-proportional layout's locators (mesh_bake.h).  The fill pass is given R and tiles alone: the cells cover the first `tiles` tiles
// of the Z-order curve
struct SizedCells {
    uint32_t R, tiles;
    static constexpr bool FILL_FLAGS = false;
    __device__ __forceinline__ bool stored(uint32_t e) const {
        const uint32_t Y = e / R, X = e - Y * R;
        return (sz_spread_bits(X >> 2) | (sz_spread_bits(Y >> 2) << 1)) < tiles;
    }
};

// the points and the store pass: the plan and the cell -> faces table
struct SizedTexels : SizedPlan {
    const int32_t *owner;
    typedef CellTexel Texel;

    template <bool FACE>
    __device__ __forceinline__ bool find(uint32_t t, CellTexel &tx) const {
        uint32_t cell, o;
        sz_texel(*this, t, cell, o, tx.s, tx.i, tx.j);
        tx.f = owner[2 * (uint64_t)cell + at_side(tx.i, tx.j, tx.s)];
        tx.e = (4 * sz_even_bits(o >> 1) + tx.j) * R + 4 * sz_even_bits(o) + tx.i;   // o < tiles <= (R / 4)^2: inside the image
        return true;
    }
    __device__ __forceinline__ bool bary(const CellTexel &tx, float &w1, float &w2, int &corner) const {
        return at_cell_bary(tx, w1, w2, corner);
    }
};

// the checks the passes after the host read share: the plan of counts_host and the carved workspace
int sz_check(uint32_t F, uint32_t R, const uint32_t *counts_host, void *ws, uint64_t ws_bytes, SizedPlan &pl, SizedPtr &p) {
    if (!counts_host) return CNERF_ENULL;
    if (const int rc = sz_plan(F, R, counts_host, &pl)) return rc;
    if (!ws) return CNERF_ENULL;
    return mesh_check_ws(ws, ws_bytes, sz_carve(ws, F, p));
}

// the same for a bake pass: the locator and the cell texels it covers
int sz_locate(uint32_t F, uint32_t R, const uint32_t *counts_host, void *ws, uint64_t ws_bytes, SizedTexels &loc, uint64_t &total) {
    SizedPtr p;
    if (const int rc = sz_check(F, R, counts_host, ws, ws_bytes, loc, p)) return rc;
    loc.owner = p.owner;
    total = 16 * (uint64_t)loc.tiles;
    return CNERF_OK;
}

}  // namespace

extern "C" {

int cnerf_mesh_atlas_layout(uint32_t F, uint32_t R, uint32_t *n_host, uint32_t *s_host) {
    if (!n_host || !s_host) return CNERF_ENULL;
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    *n_host = g.n;
    *s_host = g.s;
    return CNERF_OK;
}

int cnerf_mesh_atlas_uvs(const int32_t *faces, uint32_t V, uint32_t F, uint32_t R, float *uvs, uint32_t max_faces, uint32_t *flags,
                         void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    if (V >= (1u << 31)) return CNERF_EINVAL;
    if (!flags || (F && !faces) || (max_faces && F && !uvs)) return CNERF_ENULL;
    if (const int rc = (int)hipMemsetAsync(flags, 0, sizeof(uint32_t), CN_STREAM(stream))) return rc;
    if (F)
        hipLaunchKernelGGL(k_atlas_uvs, dim3(cn_div_up(3 * F, AT_BLOCK)), dim3(AT_BLOCK), 0, CN_STREAM(stream), faces, V, g, uvs, max_faces,
                           flags);
    return cn_launch_status();
}

int cnerf_mesh_atlas_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, uint32_t t0,
                            uint32_t t1, const uint32_t *flags, float *x, float *d, uint32_t max_points, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    if (V >= (1u << 31)) return CNERF_EINVAL;
    return bake_launch_points(g, (uint64_t)g.P * g.s * g.s, verts, normals, V, faces, t0, t1, flags, x, d, max_points, stream);
}

int cnerf_mesh_atlas_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                            const float *tangents, uint32_t t0, uint32_t t1, const float *m, uint32_t m_stride, const uint32_t *flags, float *rgb,
                            uint32_t max_points, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    if (V >= (1u << 31)) return CNERF_EINVAL;
    return bake_launch_tspace(g, (uint64_t)g.P * g.s * g.s, verts, normals, V, faces, tangents, t0, t1, m, m_stride, flags, rgb, max_points,
                              stream);
}

int cnerf_mesh_atlas_store(uint32_t F, uint32_t R, uint32_t t0, uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host,
                           const uint32_t *flags, uint8_t *image, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    return bake_launch_store(g, (uint64_t)g.P * g.s * g.s, t0, t1, rgb, rgb_stride, fill_host, flags, image, stream);
}

int cnerf_mesh_atlas_fill(uint32_t F, uint32_t R, const uint8_t *fill_host, uint8_t *image, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    return bake_launch_fill(g, fill_host, nullptr, image, stream);
}

int cnerf_mesh_atlas_sized_workspace_bytes(uint32_t F, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (F > SZ_MAX_F) return CNERF_EINVAL;
    SizedPtr p;
    *bytes_host = sz_carve(nullptr, F, p);
    return CNERF_OK;
}

int cnerf_mesh_atlas_sized_measure(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes,
                                   uint32_t *hist, void *stream) {
    if (F > SZ_MAX_F || V >= (1u << 31)) return CNERF_EINVAL;
    if (!ws || !hist || (F && (!faces || !verts))) return CNERF_ENULL;
    SizedPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, sz_carve(ws, F, p))) return rc;
    if (const int rc = (int)hipMemsetAsync(hist, 0, (SZ_BINS + 1) * sizeof(uint32_t), CN_STREAM(stream))) return rc;
    if (F) hipLaunchKernelGGL(k_sized_measure, mesh_grid(F), dim3(MC_BLOCK), 0, CN_STREAM(stream), verts, V, faces, F, p.key, hist);
    return cn_launch_status();
}

int cnerf_mesh_atlas_sized_layout(const uint32_t *hist_host, uint32_t R, uint32_t *e_host, uint32_t *counts_host, uint32_t *tiles_host) {
    if (!hist_host || !e_host || !counts_host || !tiles_host) return CNERF_ENULL;
    const int l = sz_log2(R);
    if (l < 0) return CNERF_EINVAL;
    const uint32_t K = (uint32_t)(l - 2 < 7 ? l - 2 : 7);
    uint64_t below[SZ_BINS + 1];                             // below[i] = faces with key < i
    below[0] = 0;
    for (uint32_t i = 0; i < SZ_BINS; ++i) below[i + 1] = below[i] + hist_host[i];
    const uint64_t F = below[SZ_BINS], cap = (uint64_t)(R / 4) * (R / 4);
    if (F > SZ_MAX_F) return CNERF_EINVAL;
    for (uint32_t e = 0; e <= SZ_BINS; ++e) {                // tiles(e) can rise by a cell when a face moves down a class: no bisection
        uint32_t n[SZ_CLASSES] = {0};
        uint32_t lo = 0;                                     // class k holds the keys in [lo, hi): class 0 from 0, class K up to the last bin
        for (uint32_t k = 0; k <= K; ++k) {
            const uint32_t end = e + 16 * (k + 1), hi = (k == K || end > SZ_BINS) ? SZ_BINS : end;
            n[k] = (uint32_t)(below[hi] - below[lo]);
            lo = hi;
        }
        const uint64_t t = sz_tiles(n);
        if (t <= cap) {
            *e_host = e;
            *tiles_host = (uint32_t)t;
            for (int k = 0; k < SZ_CLASSES; ++k) counts_host[k] = n[k];
            return CNERF_OK;
        }
    }
    return CNERF_EINVAL;                                     // even one 4 x 4 cell per face pair does not fit: decimate or raise R
}

int cnerf_mesh_atlas_sized_plan(uint32_t F, uint32_t R, uint32_t e, const uint32_t *counts_host, void *ws, uint64_t ws_bytes,
                                const uint32_t *flags, int32_t *cells, uint32_t max_faces, void *stream) {
    SizedPlan pl;
    SizedPtr p;
    if (e > SZ_BINS) return CNERF_EINVAL;
    if (const int rc = sz_check(F, R, counts_host, ws, ws_bytes, pl, p)) return rc;
    if (!F) return CNERF_OK;
    if (!flags || (max_faces && !cells)) return CNERF_ENULL;
    const dim3 grid = mesh_grid(F);
    if (const int rc = (int)hipMemsetAsync(p.owner, 0xff, 2 * (uint64_t)F * sizeof(int32_t), CN_STREAM(stream))) return rc;
    hipLaunchKernelGGL(k_sized_count, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), pl, e, p);
    hipLaunchKernelGGL(k_sized_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, CN_STREAM(stream), grid.x, p);
    hipLaunchKernelGGL(k_sized_emit, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), pl, e, p, flags, cells, max_faces);
    return cn_launch_status();
}

int cnerf_mesh_atlas_sized_uvs(uint32_t F, uint32_t R, const int32_t *cells, const uint32_t *flags, float *uvs, uint32_t max_faces,
                               void *stream) {
    if (sz_log2(R) < 0 || F > SZ_MAX_F) return CNERF_EINVAL;
    const uint32_t n = F < max_faces ? F : max_faces;
    if (!n) return CNERF_OK;
    if (!cells || !flags || !uvs) return CNERF_ENULL;
    hipLaunchKernelGGL(k_sized_uvs, dim3(cn_div_up(3 * n, AT_BLOCK)), dim3(AT_BLOCK), 0, CN_STREAM(stream), n, R, cells, flags, uvs);
    return cn_launch_status();
}

int cnerf_mesh_atlas_sized_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                                  const uint32_t *counts_host, void *ws, uint64_t ws_bytes, uint32_t t0, uint32_t t1,
                                  const uint32_t *flags, float *x, float *d, uint32_t max_points, void *stream) {
    SizedTexels loc;
    uint64_t total;
    if (const int rc = sz_locate(F, R, counts_host, ws, ws_bytes, loc, total)) return rc;
    if (V >= (1u << 31)) return CNERF_EINVAL;
    return bake_launch_points(loc, total, verts, normals, V, faces, t0, t1, flags, x, d, max_points, stream);
}

int cnerf_mesh_atlas_sized_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                                  const uint32_t *counts_host, void *ws, uint64_t ws_bytes, const float *tangents, uint32_t t0, uint32_t t1,
                                  const float *m, uint32_t m_stride, const uint32_t *flags, float *rgb, uint32_t max_points, void *stream) {
    SizedTexels loc;
    uint64_t total;
    if (const int rc = sz_locate(F, R, counts_host, ws, ws_bytes, loc, total)) return rc;
    if (V >= (1u << 31)) return CNERF_EINVAL;
    return bake_launch_tspace(loc, total, verts, normals, V, faces, tangents, t0, t1, m, m_stride, flags, rgb, max_points, stream);
}

int cnerf_mesh_atlas_sized_store(uint32_t F, uint32_t R, const uint32_t *counts_host, void *ws, uint64_t ws_bytes, uint32_t t0,
                                 uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host, const uint32_t *flags,
                                 uint8_t *image, void *stream) {
    SizedTexels loc;
    uint64_t total;
    if (const int rc = sz_locate(F, R, counts_host, ws, ws_bytes, loc, total)) return rc;
    return bake_launch_store(loc, total, t0, t1, rgb, rgb_stride, fill_host, flags, image, stream);
}

int cnerf_mesh_atlas_sized_fill(uint32_t R, uint32_t tiles, const uint8_t *fill_host, uint8_t *image, void *stream) {
    if (sz_log2(R) < 0 || (uint64_t)tiles > (uint64_t)(R / 4) * (R / 4)) return CNERF_EINVAL;
    return bake_launch_fill(SizedCells{R, tiles}, fill_host, nullptr, image, stream);
}

}  // extern "C"
