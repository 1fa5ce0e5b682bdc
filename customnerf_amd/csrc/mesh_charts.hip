// Chart-based texture atlas of a triangle mesh (cnerf_mesh_atlas_proj_*; bake_texture(layout='projected')): faces are grouped into charts by
// the dominant axis of their normal, every chart is projected along its axis, the charts are shelf-packed at one texel density, texels find
// their face by an exact rasterisation in UV space and a gutter is grown round every chart.  Same conventions as the other mesh passes: the
// caller's stream and workspace, no allocation, three host reads (the counts, the C extents, the totals), integer atomics only (the output is bit-reproducible).  The rules are in
// include/customnerf_hip.h; the NumPy restatement the tests pin them to: tests/atlas_proj_restatement.py.
//
//   k_pj_nodes    : one thread per node 6 v + class: parent = itself, unused
//   k_pj_class    : one thread per face: its class (own axis, or the vertex normals' when that keeps it front-facing), the index check;
//                   marks its three nodes and unites them (cc_union of mesh_common.h: a root is its component's smallest node)
//   k_pj_compress : every node -> its root
//   k_pj_root_count / _scan / _emit : chart index = rank of the root among the used roots (the scans of mesh_common.h); empty extents
//   k_pj_extents  : one thread per face: its chart, min / max of its projected corners by integer atomics on the ordered image of the float
//   k_pj_finish   : the charts' extents as floats and C: the host reads C, then C extents; cnerf_mesh_atlas_proj_pack packs them on the host
//   k_pj_uvs      : one thread per face: its corners in texel space in fp64 -> UVs and the corners snapped to 1 / 256 texel
//   k_pj_cover    : pass A (texel centres inside, edges inclusive) and pass B (conservative, on texels A left) as atomicMin of the face
//                   index; one thread per face, which puts a face whose box has more than PJ_BIG texels on a list that k_pj_cover_big
//                   covers a workgroup per face (the minimum does not depend on which path claimed a texel, nor on the list's order);
//                   pass B also counts the strictly covered texels another face owns
//   k_pj_merge / k_pj_grow : A's owner, else B's; then one Jacobi round per gutter texel
//   k_pj_list_count / _scan / _emit : owned texels in row-major order -> the texel list; the last host read (total, overlap_texels)
//   k_bake_points / _store / _fill<PjTexels> : the bake of mesh_bake.h (once k_pj_points / k_pj_store / k_pj_fill), for listed texels
#include "mesh_bake.h"

#define PJ_BLOCK BK_BLOCK
#define PJ_BAD_INDEX 1u
#define PJ_MAX_V (1u << 28)                                  // 6 V nodes fit 32 bits
#define PJ_MAX_F (1u << 26)
#define PJ_MAX_GUTTER 8u
#define PJ_NONE 0x7f7f7f7f                                   // what hipMemset(0x7f) leaves: above every face index
#define PJ_BIG 1024u                                         // box texels above which a face is covered by a workgroup
#define PJ_BIG_GRID 1024u                                    // workgroups that share the large faces
#define PJ_UNCHARTED INT32_MIN

namespace {

struct PjPtr {
    uint32_t *hdr, *parent, *rank, *sums, *ext, *list, *big;  // hdr[0] = C, hdr[1] = total, hdr[2 + PASS] = the large faces of a pass; big [2][F]
    int32_t *fclass, *fchart, *snap, *map_a, *map_b;
    uint64_t nsum;
};

uint64_t pj_carve(void *ws, uint64_t V, uint64_t F, uint64_t R, PjPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.parent = c.take<uint32_t>(6 * V);
    p.rank = c.take<uint32_t>(6 * V);
    const uint64_t n = 6 * V > R * R ? 6 * V : R * R;
    p.nsum = cn_div_up64(n ? n : 1, MC_BLOCK);
    p.sums = c.take<uint32_t>(p.nsum);
    p.ext = c.take<uint32_t>(4 * F);
    p.fclass = c.take<int32_t>(F);
    p.fchart = c.take<int32_t>(F);
    p.snap = c.take<int32_t>(6 * F);
    p.map_a = c.take<int32_t>(R * R);
    p.map_b = c.take<int32_t>(R * R);
    p.list = c.take<uint32_t>(R * R);
    p.big = c.take<uint32_t>(2 * F);
    return c.total();
}

int pj_check(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, PjPtr &p) {
    if (V > PJ_MAX_V || F > PJ_MAX_F || R < 16 || R > 16384) return CNERF_EINVAL;
    if (!ws) return CNERF_ENULL;
    return mesh_check_ws(ws, ws_bytes, pj_carve(ws, V, F, R, p));
}

// the order-preserving integer image of a float and back
__device__ __forceinline__ uint32_t pj_enc(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float pj_dec(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? u ^ 0x80000000u : ~u); }

// axis of the largest |c_k| (ties to the lowest k) and the sign of that component: 2 k + (c_k < 0)
__device__ __forceinline__ uint32_t pj_axis(const float c[3]) {
    uint32_t k = 0;
    if (fabsf(c[1]) > fabsf(c[0])) k = 1;
    if (fabsf(c[2]) > fabsf(c[k])) k = 2;
    return 2 * k + (c[k] < 0.0f ? 1u : 0u);
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_nodes(uint32_t N, PjPtr p) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < N) {
        p.parent[i] = i;
        p.rank[i] = 0;
    }
    if (i < 2) p.hdr[i] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_class(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                       const int32_t *__restrict__ faces, uint32_t F, PjPtr p, uint32_t *__restrict__ flags) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    if (!mesh_face(faces, f, V, t)) {
        atomicOr(flags, PJ_BAD_INDEX);
        p.fclass[f] = 6;
        return;
    }
    float a[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) at_load3(verts, t[q], a[q]);
    const float e1[3] = {a[1][0] - a[0][0], a[1][1] - a[0][1], a[1][2] - a[0][2]};
    const float e2[3] = {a[2][0] - a[0][0], a[2][1] - a[0][1], a[2][2] - a[0][2]};
    const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float q = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    uint32_t cls = 6;
    if (q > 0.0f && q < INFINITY) {
        cls = pj_axis(c);
        if (normals) {
            float n[3][3], g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) at_load3(normals, t[k], n[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = (n[0][k] + n[1][k]) + n[2][k];
            const bool finite = fabsf(g[0]) < INFINITY && fabsf(g[1]) < INFINITY && fabsf(g[2]) < INFINITY;   // false for a NaN
            if (finite && (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f)) {
                const uint32_t gc = pj_axis(g), k = gc >> 1;
                const float ck = c[k];
                if ((ck < 0.0f) == (bool)(gc & 1u) && 4.0f * (ck * ck) >= q) cls = gc;
            }
        }
    }
    p.fclass[f] = (int32_t)cls;
    if (cls == 6) return;
    const uint32_t n0 = 6 * t[0] + cls, n1 = 6 * t[1] + cls, n2 = 6 * t[2] + cls;
    st_rlx(p.rank + n0, 1u);                                 // used: every writer stores 1
    st_rlx(p.rank + n1, 1u);
    st_rlx(p.rank + n2, 1u);
    cc_union(p.parent, n0, n1);
    cc_union(p.parent, n1, n2);
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_compress(uint32_t N, uint32_t *parent) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= N) return;
    uint32_t r = ld_rlx(parent + v), n;
    while ((n = ld_rlx(parent + r)) != r) r = n;             // the forest is final: concurrent writers only store roots
    st_rlx(parent + v, r);
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_root_count(uint32_t N, PjPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t tot = mc_block_total<1>(i < N && p.rank[i] && p.parent[i] == i ? 1u : 0u, red);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = tot;
}

// one workgroup: the workgroup totals -> exclusive offsets; hdr[slot] = the total
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_pj_scan(uint32_t nblk, PjPtr p, uint32_t slot) {
    uint64_t tot[1];
    mc_scan_totals_n<1>(p.sums, nblk, tot);
    if (threadIdx.x == 0) p.hdr[slot] = (uint32_t)tot[0];
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_root_emit(uint32_t N, uint32_t F, PjPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t root = i < N && p.rank[i] && p.parent[i] == i ? 1u : 0u;
    const uint32_t r = p.sums[blockIdx.x] + mc_block_prefix<1>(root, red);
    if (!root || r >= F) return;                             // a chart has a face: C <= F
    p.rank[i] = r;
    uint32_t *e = p.ext + 4 * (uint64_t)r;                   // a0, a1, b0, b1: empty
    e[0] = 0xffffffffu;
    e[1] = 0u;
    e[2] = 0xffffffffu;
    e[3] = 0u;
}

// the projected (a, b) of a point for a class < 6
__device__ __forceinline__ void pj_project(uint32_t cls, const float x[3], float &a, float &b) {
    const uint32_t k = cls >> 1, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    a = x[(cls & 1u) ? k2 : k1];
    b = x[(cls & 1u) ? k1 : k2];
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_extents(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ faces,
                                                         uint32_t F, PjPtr p, const uint32_t *__restrict__ flags,
                                                         int32_t *__restrict__ face_class, int32_t *__restrict__ face_chart,
                                                         uint32_t max_faces) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F || flags[0]) return;                          // after a bad index nothing is written
    const uint32_t cls = (uint32_t)p.fclass[f];
    int32_t chart = -1;
    if (cls < 6) {
        uint32_t t[3];
        mesh_face(faces, f, V, t);                           // in range: no flag
        const uint32_t r = p.rank[p.parent[6 * t[0] + cls]];
        if (r < F) {
            chart = (int32_t)r;
            uint32_t *e = p.ext + 4 * (uint64_t)r;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float x[3], a, b;
                at_load3(verts, t[q], x);
                pj_project(cls, x, a, b);
                const uint32_t ia = pj_enc(a), ib = pj_enc(b);           // most corners move no bound: a bound only ever moves outwards, so
                if (ia < ld_rlx(e)) atomicMin(e, ia);                    // a stale read can only let a needless atomic through
                if (ia > ld_rlx(e + 1)) atomicMax(e + 1, ia);
                if (ib < ld_rlx(e + 2)) atomicMin(e + 2, ib);
                if (ib > ld_rlx(e + 3)) atomicMax(e + 3, ib);
            }
        }
    }
    p.fchart[f] = chart;
    if (f >= max_faces) return;
    face_class[f] = (int32_t)cls;
    face_chart[f] = chart;
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_finish(PjPtr p, const uint32_t *__restrict__ flags, uint32_t *__restrict__ counts,
                                                        float *__restrict__ extents, uint32_t max_charts) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (flags[0]) return;
    const uint32_t C = p.hdr[0];
    if (i == 0) counts[0] = C;
    if (i >= C || i >= max_charts) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) extents[4 * (uint64_t)i + q] = pj_dec(p.ext[4 * (uint64_t)i + q]);
}

struct PjGeom {
    uint32_t F, R, C, g;
    double rho;
};

__global__ __launch_bounds__(PJ_BLOCK) void k_pj_uvs(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ faces, PjGeom G,
                                                     const int32_t *__restrict__ rects, PjPtr p, const uint32_t *__restrict__ flags,
                                                     float *__restrict__ uvs, uint32_t max_faces) {
    const uint32_t f = blockIdx.x * PJ_BLOCK + threadIdx.x;
    if (f >= G.F || flags[0]) return;
    const int32_t chart = p.fchart[f];
    const uint32_t cls = (uint32_t)p.fclass[f];
    int32_t *sn = p.snap + 6 * (uint64_t)f;
    float *uv = uvs + 6 * (uint64_t)f;
    uint32_t t[3];
    if (chart < 0 || (uint32_t)chart >= G.C || cls >= 6 || !mesh_face(faces, f, V, t)) {
        sn[0] = PJ_UNCHARTED;
        if (f < max_faces) {
#pragma unroll
            for (int q = 0; q < 6; ++q) uv[q] = 0.0f;
        }
        return;
    }
    const int32_t *rc = rects + 4 * (uint64_t)chart;
    const uint32_t *e = p.ext + 4 * (uint64_t)chart;
    const double a0 = (double)pj_dec(e[0]), b0 = (double)pj_dec(e[2]);
    const double ox = (double)(rc[0] + (int32_t)G.g) + 0.5, oy = (double)(rc[1] + rc[3] - 1 - (int32_t)G.g) + 0.5, Rd = (double)G.R;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float x[3], a, b;
        at_load3(verts, t[q], x);
        pj_project(cls, x, a, b);
        const double tx = ox + G.rho * ((double)a - a0), ty = oy - G.rho * ((double)b - b0);
        sn[2 * q] = (int32_t)rint(256.0 * tx);
        sn[2 * q + 1] = (int32_t)rint(256.0 * ty);
        if (f < max_faces) {
            uv[2 * q] = (float)(tx / Rd);
            uv[2 * q + 1] = (float)(1.0 - ty / Rd);
        }
    }
}

// the snapped corners of a charted face, its doubled area A (positive for a face that is counter-clockwise with v up) and the edge functions
// E_k(px, py) = (yj - yi)(px - xi) - (xj - xi)(py - yi), i = (k + 1) % 3, j = (k + 2) % 3: E_k / A is the barycentric weight of corner k
struct PjTri {
    int64_t x[3], y[3], A;
    __device__ __forceinline__ bool load(const int32_t *__restrict__ snap, uint32_t f) {
        const int32_t *s = snap + 6 * (uint64_t)f;
        if (s[0] == PJ_UNCHARTED) return false;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            x[q] = s[2 * q];
            y[q] = s[2 * q + 1];
        }
        A = (y[1] - y[0]) * (x[2] - x[0]) - (x[1] - x[0]) * (y[2] - y[0]);
        return true;
    }
    __device__ __forceinline__ int64_t edge(int k, int64_t px, int64_t py) const {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        return (y[j] - y[i]) * (px - x[i]) - (x[j] - x[i]) * (py - y[i]);
    }
    __device__ __forceinline__ int64_t slack(int k) const {   // 128 (|dx_k| + |dy_k|): what E_k can gain inside the texel's square
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const int64_t dx = x[j] - x[i], dy = y[j] - y[i];
        return 128 * ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
    }
};

__device__ __forceinline__ int64_t pj_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
__device__ __forceinline__ int64_t pj_min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
__device__ __forceinline__ int64_t pj_max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// PASS 0 (A): centres inside, edges inclusive.  PASS 1 (B): the conservative cover on texels A left un-owned, and the overlap count.
// One thread per face (COOP false) covers a box of at most PJ_BIG texels and lists a larger face for k_pj_cover_big, where a workgroup
// (COOP true) covers it.
template <int PASS, bool COOP>
__device__ __forceinline__ void pj_cover_face(uint32_t f, const PjGeom &G, const PjPtr &p, unsigned long long *__restrict__ overlap) {
    PjTri t;
    if (!t.load(p.snap, f)) return;
    if (PASS == 0 && t.A <= 0) return;
    const int64_t minx = pj_min3(t.x[0], t.x[1], t.x[2]), maxx = pj_max3(t.x[0], t.x[1], t.x[2]);
    const int64_t miny = pj_min3(t.y[0], t.y[1], t.y[2]), maxy = pj_max3(t.y[0], t.y[1], t.y[2]);
    const int64_t last = (int64_t)G.R - 1;
    int64_t X0, X1, Y0, Y1;
    if (PASS == 0) {                                         // centres 256 X + 128 in [min, max]
        X0 = pj_floor_div(minx - 128 + 255, 256);
        X1 = pj_floor_div(maxx - 128, 256);
        Y0 = pj_floor_div(miny - 128 + 255, 256);
        Y1 = pj_floor_div(maxy - 128, 256);
    } else {                                                 // squares [256 X, 256 X + 256] meeting [min, max]
        X0 = pj_floor_div(minx - 256 + 255, 256);
        X1 = pj_floor_div(maxx, 256);
        Y0 = pj_floor_div(miny - 256 + 255, 256);
        Y1 = pj_floor_div(maxy, 256);
    }
    X0 = X0 < 0 ? 0 : X0;
    Y0 = Y0 < 0 ? 0 : Y0;
    X1 = X1 > last ? last : X1;
    Y1 = Y1 > last ? last : Y1;
    if (X1 < X0 || Y1 < Y0) return;
    const uint32_t bw = (uint32_t)(X1 - X0 + 1), n = bw * (uint32_t)(Y1 - Y0 + 1);         // <= R^2 <= 2^28
    if (!COOP && n > PJ_BIG) {                               // a workgroup's face: onto this pass's list (any order: the owner is a minimum)
        p.big[(uint64_t)PASS * G.F + atomicAdd(p.hdr + 2 + PASS, 1u)] = f;
        return;
    }
    const int64_t s0 = t.slack(0), s1 = t.slack(1), s2 = t.slack(2);
    uint32_t over = 0;
    for (uint32_t i = COOP ? threadIdx.x : 0u; i < n; i += COOP ? PJ_BLOCK : 1u) {
        const uint32_t iy = i / bw, ix = i - iy * bw;
        const int64_t X = X0 + ix, Y = Y0 + iy, px = 256 * X + 128, py = 256 * Y + 128;
        const uint64_t e = (uint64_t)Y * G.R + (uint64_t)X;
        const int64_t E0 = t.edge(0, px, py), E1 = t.edge(1, px, py), E2 = t.edge(2, px, py);
        if (PASS == 0) {
            if (E0 >= 0 && E1 >= 0 && E2 >= 0) atomicMin(p.map_a + e, (int32_t)f);
        } else {
            const int32_t own = p.map_a[e];
            if (t.A > 0 && E0 > 0 && E1 > 0 && E2 > 0 && own != (int32_t)f) ++over;
            if (own == PJ_NONE && (t.A <= 0 || (E0 + s0 >= 0 && E1 + s1 >= 0 && E2 + s2 >= 0))) atomicMin(p.map_b + e, (int32_t)f);
        }
    }
    if (PASS == 1 && over) atomicAdd(overlap, (unsigned long long)over);
}

template <int PASS>
__global__ __launch_bounds__(PJ_BLOCK) void k_pj_cover(PjGeom G, PjPtr p, const uint32_t *__restrict__ flags,
                                                       unsigned long long *__restrict__ overlap) {
    const uint32_t f = blockIdx.x * PJ_BLOCK + threadIdx.x;
    if (f >= G.F || flags[0]) return;
    pj_cover_face<PASS, false>(f, G, p, overlap);
}

// the faces k_pj_cover<PASS> listed, a workgroup at a time; with an empty list the workgroups leave at once
template <int PASS>
__global__ __launch_bounds__(PJ_BLOCK) void k_pj_cover_big(PjGeom G, PjPtr p, const uint32_t *__restrict__ flags,
                                                           unsigned long long *__restrict__ overlap) {
    if (flags[0]) return;
    const uint32_t n = p.hdr[2 + PASS];
    for (uint32_t i = blockIdx.x; i < n && i < G.F; i += gridDim.x) {
        const uint32_t f = p.big[(uint64_t)PASS * G.F + i];
        if (f < G.F) pj_cover_face<PASS, true>(f, G, p, overlap);
    }
}

// A's owner, else B's, else -1 -> dst (map_a or map_b: the same index is read and written)
__global__ __launch_bounds__(PJ_BLOCK) void k_pj_merge(uint32_t R, PjPtr p, int32_t *__restrict__ dst, const uint32_t *__restrict__ flags,
                                                       int32_t *__restrict__ owner_ab) {
    const uint32_t e = blockIdx.x * PJ_BLOCK + threadIdx.x;
    if (e >= R * R || flags[0]) return;
    const int32_t a = p.map_a[e], b = p.map_b[e], o = a != PJ_NONE ? a : b != PJ_NONE ? b : -1;
    dst[e] = o;
    if (owner_ab) owner_ab[e] = o;
}

// one Jacobi round: an un-owned texel takes the owner of its first owned neighbour in the order W, E, N, S, NW, NE, SW, SE (N: the row above)
__global__ __launch_bounds__(PJ_BLOCK) void k_pj_grow(uint32_t R, const int32_t *__restrict__ src, int32_t *__restrict__ dst,
                                                      const uint32_t *__restrict__ flags) {
    const uint32_t e = blockIdx.x * PJ_BLOCK + threadIdx.x;
    if (e >= R * R || flags[0]) return;
    const int32_t Y = (int32_t)(e / R), X = (int32_t)(e - (uint32_t)Y * R);
    int32_t o = src[e];
    const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int32_t x = X + dx[k], y = Y + dy[k];
        if (o < 0 && x >= 0 && y >= 0 && x < (int32_t)R && y < (int32_t)R) o = src[(uint64_t)y * R + (uint32_t)x];
    }
    dst[e] = o;
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_list_count(uint32_t R, PjPtr p, const uint32_t *__restrict__ flags) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t e = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t tot = mc_block_total<1>(e < R * R && !flags[0] && p.map_a[e] >= 0 ? 1u : 0u, red);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MC_BLOCK) void k_pj_list_emit(uint32_t R, PjPtr p, const uint32_t *__restrict__ flags, int32_t *__restrict__ owner,
                                                           unsigned long long *__restrict__ totals) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t e = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool in = e < R * R && !flags[0];
    const int32_t o = in ? p.map_a[e] : -1;
    const uint32_t r = p.sums[blockIdx.x] + mc_block_prefix<1>(o >= 0 ? 1u : 0u, red);
    if (!in) return;
    if (e == 0) totals[0] = p.hdr[1];
    owner[e] = o;
    if (o >= 0) p.list[r] = e;
}

// The locator of the bake (mesh_bake.h): cell texel t is entry t of the texel list, owned by the face map_a names.  A face whose snapped
// triangle has no area is baked at its vertex 0.
struct PjTexels {
    uint32_t F, R;
    const uint32_t *hdr, *list;
    const int32_t *map_a, *snap;
    struct Texel {
        uint32_t e;
        int32_t f;
    };
    static constexpr bool FILL_FLAGS = true;

    // the store pass reads neither the owner map nor the snapped corners: every listed texel is owned
    template <bool FACE>
    __device__ __forceinline__ bool find(uint32_t t, Texel &tx) const {
        if (t >= hdr[1]) return false;
        tx.e = list[t];
        if (tx.e >= R * R) return false;
        tx.f = FACE ? map_a[tx.e] : 0;
        return !FACE || (tx.f >= 0 && (uint32_t)tx.f < F && snap[6 * (uint64_t)tx.f] != PJ_UNCHARTED);
    }
    __device__ __forceinline__ bool bary(const Texel &tx, float &w1, float &w2, int &corner) const {
        PjTri tri;
        tri.load(snap, (uint32_t)tx.f);                      // charted: find looked
        w1 = w2 = 0.0f;
        corner = -1;
        if (tri.A <= 0) return false;
        const uint32_t Y = tx.e / R, X = tx.e - Y * R;
        const int64_t px = 256 * (int64_t)X + 128, py = 256 * (int64_t)Y + 128;
        w1 = (float)((double)tri.edge(1, px, py) / (double)tri.A);
        w2 = (float)((double)tri.edge(2, px, py) / (double)tri.A);
        return true;
    }
    __device__ __forceinline__ bool stored(uint32_t e) const { return map_a[e] >= 0; }
};

// the checks the bake passes share, and their locator
int pj_locate(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, PjTexels &loc) {
    PjPtr p;
    if (const int rc = pj_check(V, F, R, ws, ws_bytes, p)) return rc;
    loc = {F, R, p.hdr, p.list, p.map_a, p.snap};
    return CNERF_OK;
}

// host: the shelf packing of C charts at density rho; false when it does not fit.  ord = the charts by h, then w, descending, then index
struct PjPack {
    uint32_t C, R, g;
    const float *ext;
    double *sw, *sh;                                         // [C] sizes at the density in hand
    uint32_t *ord, *tmp, *cnt;                               // [C], [C], [R + 1]

    void sizes(double rho) {
        for (uint32_t c = 0; c < C; ++c) {
            const double da = (double)ext[4 * c + 1] - (double)ext[4 * c], db = (double)ext[4 * c + 3] - (double)ext[4 * c + 2];
            sw[c] = ceil(rho * da) + 1.0 + 2.0 * g;
            sh[c] = ceil(rho * db) + 1.0 + 2.0 * g;
        }
    }
    // one stable counting pass, keys (integers in [1, R]) descending: src (nullptr: the identity) -> dst
    void pass(const double *key, const uint32_t *src, uint32_t *dst) {
        for (uint32_t i = 0; i <= R; ++i) cnt[i] = 0;
        for (uint32_t c = 0; c < C; ++c) ++cnt[R - (uint32_t)key[src ? src[c] : c]];
        uint32_t at = 0;
        for (uint32_t i = 0; i <= R; ++i) {
            const uint32_t n = cnt[i];
            cnt[i] = at;
            at += n;
        }
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t id = src ? src[c] : c;
            dst[cnt[R - (uint32_t)key[id]]++] = id;
        }
    }
    void sort() {                                            // by w, then stably by h: index order survives inside equal (h, w)
        pass(sw, nullptr, tmp);
        pass(sh, tmp, ord);
    }
    bool fit(double rho, int32_t *rects) {
        sizes(rho);
        for (uint32_t c = 0; c < C; ++c)
            if (!(sw[c] <= (double)R && sh[c] <= (double)R)) return false;   // also a NaN
        sort();
        int64_t x = 0, y = 0, shelf = C ? (int64_t)sh[ord[0]] : 0;
        for (uint32_t i = 0; i < C; ++i) {
            const uint32_t c = ord[i];
            const int64_t w = (int64_t)sw[c], h = (int64_t)sh[c];
            if (x + w > (int64_t)R) {
                y += shelf;
                x = 0;
                shelf = h;
            }
            if (y + shelf > (int64_t)R) return false;
            if (rects) {
                rects[4 * c] = (int32_t)x;
                rects[4 * c + 1] = (int32_t)y;
                rects[4 * c + 2] = (int32_t)w;
                rects[4 * c + 3] = (int32_t)h;
            }
            x += w;
        }
        return true;
    }
};

}  // namespace

extern "C" {

int cnerf_mesh_atlas_proj_workspace_bytes(uint32_t V, uint32_t F, uint32_t R, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (V > PJ_MAX_V || F > PJ_MAX_F || R < 16 || R > 16384) return CNERF_EINVAL;
    PjPtr p;
    *bytes_host = pj_carve(nullptr, V, F, R, p);
    return CNERF_OK;
}

int cnerf_mesh_atlas_proj_charts(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, uint32_t *counts, int32_t *face_class, int32_t *face_chart, uint32_t max_faces,
                                 float *extents, uint32_t max_charts, void *stream) {
    PjPtr p;
    if (const int rc = pj_check(V, F, R, ws, ws_bytes, p)) return rc;
    if (!counts || (F && (!faces || !verts)) || (F && max_faces && (!face_class || !face_chart)) || (F && max_charts && !extents))
        return CNERF_ENULL;
    hipStream_t s = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s)) return rc;
    uint32_t *flags = counts + 1;
    const uint32_t N = 6 * V;
    hipLaunchKernelGGL(k_pj_nodes, mesh_grid(N > 2 ? N : 2), dim3(MC_BLOCK), 0, s, N, p);
    if (!F) return cn_launch_status();
    hipLaunchKernelGGL(k_pj_class, mesh_grid(F), dim3(MC_BLOCK), 0, s, verts, normals, V, faces, F, p, flags);
    const dim3 gn = mesh_grid(N);                            // F > 0 and an index in range need V > 0; V = 0 flags every face
    if (N) {
        hipLaunchKernelGGL(k_pj_compress, gn, dim3(MC_BLOCK), 0, s, N, p.parent);
        hipLaunchKernelGGL(k_pj_root_count, gn, dim3(MC_BLOCK), 0, s, N, p);
        hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, s, gn.x, p, 0u);
        hipLaunchKernelGGL(k_pj_root_emit, gn, dim3(MC_BLOCK), 0, s, N, F, p);
    }
    hipLaunchKernelGGL(k_pj_extents, mesh_grid(F), dim3(MC_BLOCK), 0, s, verts, V, faces, F, p, flags, face_class, face_chart, max_faces);
    hipLaunchKernelGGL(k_pj_finish, mesh_grid(F), dim3(MC_BLOCK), 0, s, p, flags, counts, extents, max_charts);
    return cn_launch_status();
}

int cnerf_mesh_atlas_proj_pack(const float *extents_host, uint32_t C, uint32_t R, uint32_t gutter, double *rho_host, int32_t *rects_host) {
    if (!rho_host || (C && (!extents_host || !rects_host))) return CNERF_ENULL;
    if (R < 16 || R > 16384 || gutter > PJ_MAX_GUTTER || C > PJ_MAX_F) return CNERF_EINVAL;
    *rho_host = 0.0;
    if (!C) return CNERF_OK;
    const double side = 1.0 + 2.0 * gutter;                  // more charts than cells of the smallest size: no packing, and no scratch for one
    if ((double)C > floor((double)R / side) * floor((double)R / side)) return CNERF_EINVAL;
    double *sw = (double *)malloc(2 * (size_t)C * sizeof(double));
    uint32_t *ord = (uint32_t *)malloc((2 * (size_t)C + R + 1) * sizeof(uint32_t));
    if (!sw || !ord) {
        free(sw);
        free(ord);
        return (int)hipErrorOutOfMemory;                     // not CNERF_EINVAL: that says the charts do not fit
    }
    PjPack pk = {C, R, gutter, extents_host, sw, sw + C, ord, ord + C, ord + 2 * (size_t)C};
    double big = 0.0;
    bool ok = true;
    for (uint32_t c = 0; c < C && ok; ++c) {
        const double da = (double)extents_host[4 * c + 1] - (double)extents_host[4 * c];
        const double db = (double)extents_host[4 * c + 3] - (double)extents_host[4 * c + 2];
        ok = da >= 0.0 && db >= 0.0 && da < (double)INFINITY && db < (double)INFINITY;       // false for a NaN
        big = da > big ? da : big;
        big = db > big ? db : big;
    }
    int rc = CNERF_EINVAL;
    if (ok && pk.fit(0.0, rects_host)) {
        rc = CNERF_OK;
        double rho = 0.0;
        const double hi0 = big > 0.0 ? ((double)R - 1.0 - 2.0 * gutter) / big : 0.0;
        if (hi0 > 0.0 && hi0 < (double)INFINITY) {
            if (pk.fit(hi0, nullptr)) {
                rho = hi0;
            } else {
                double lo = 0.0, hi = hi0;
                for (int it = 0; it < 24; ++it) {
                    const double mid = 0.5 * (lo + hi);
                    if (pk.fit(mid, nullptr)) lo = mid;
                    else hi = mid;
                }
                rho = lo;
            }
        }
        pk.fit(rho, rects_host);
        *rho_host = rho;
    }
    free(sw);
    free(ord);
    return rc;
}

int cnerf_mesh_atlas_proj_raster(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, uint32_t gutter, double rho,
                                 const int32_t *rects, uint32_t C, void *ws, uint64_t ws_bytes, const uint32_t *flags, float *uvs,
                                 uint32_t max_faces, int32_t *owner_ab, int32_t *owner, uint64_t *totals, void *stream) {
    PjPtr p;
    if (const int rc = pj_check(V, F, R, ws, ws_bytes, p)) return rc;
    if (gutter > PJ_MAX_GUTTER || C > F || !(rho >= 0.0 && rho < (double)INFINITY)) return CNERF_EINVAL;
    if (!flags || !owner || !totals || (F && (!faces || !verts)) || (C && !rects) || (F && max_faces && !uvs)) return CNERF_ENULL;
    hipStream_t s = CN_STREAM(stream);
    const uint64_t map_bytes = (uint64_t)R * R * sizeof(int32_t);
    if (const int rc = (int)hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), s)) return rc;
    if (const int rc = (int)hipMemsetAsync(p.hdr + 2, 0, 2 * sizeof(uint32_t), s)) return rc;     // the two lists of large faces: empty
    if (const int rc = (int)hipMemsetAsync(p.map_a, 0x7f, map_bytes, s)) return rc;
    if (const int rc = (int)hipMemsetAsync(p.map_b, 0x7f, map_bytes, s)) return rc;
    const PjGeom G = {F, R, C, gutter, rho};
    unsigned long long *tot = (unsigned long long *)totals;
    if (F) {
        const dim3 gf(cn_div_up(F, PJ_BLOCK));
        hipLaunchKernelGGL(k_pj_uvs, gf, dim3(PJ_BLOCK), 0, s, verts, V, faces, G, rects, p, flags, uvs, max_faces);
        const dim3 gb(F < PJ_BIG_GRID ? F : PJ_BIG_GRID);
        hipLaunchKernelGGL(k_pj_cover<0>, gf, dim3(PJ_BLOCK), 0, s, G, p, flags, tot + 1);
        hipLaunchKernelGGL(k_pj_cover_big<0>, gb, dim3(PJ_BLOCK), 0, s, G, p, flags, tot + 1);
        hipLaunchKernelGGL(k_pj_cover<1>, gf, dim3(PJ_BLOCK), 0, s, G, p, flags, tot + 1);
        hipLaunchKernelGGL(k_pj_cover_big<1>, gb, dim3(PJ_BLOCK), 0, s, G, p, flags, tot + 1);
    }
    const dim3 gt(cn_div_up(R * R, PJ_BLOCK));
    int32_t *cur = (gutter & 1u) ? p.map_b : p.map_a, *oth = (gutter & 1u) ? p.map_a : p.map_b;    // the last round ends in map_a
    hipLaunchKernelGGL(k_pj_merge, gt, dim3(PJ_BLOCK), 0, s, R, p, cur, flags, owner_ab);
    for (uint32_t r = 0; r < gutter; ++r) {
        hipLaunchKernelGGL(k_pj_grow, gt, dim3(PJ_BLOCK), 0, s, R, cur, oth, flags);
        int32_t *t = cur;
        cur = oth;
        oth = t;
    }
    const dim3 gl = mesh_grid((uint64_t)R * R);
    hipLaunchKernelGGL(k_pj_list_count, gl, dim3(MC_BLOCK), 0, s, R, p, flags);
    hipLaunchKernelGGL(k_pj_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, s, gl.x, p, 1u);
    hipLaunchKernelGGL(k_pj_list_emit, gl, dim3(MC_BLOCK), 0, s, R, p, flags, owner, tot);
    return cn_launch_status();
}

int cnerf_mesh_atlas_proj_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, uint32_t t0, uint32_t t1, const uint32_t *flags, float *x, float *d, uint32_t max_points,
                                 void *stream) {
    PjTexels loc;
    if (const int rc = pj_locate(V, F, R, ws, ws_bytes, loc)) return rc;
    return bake_launch_points(loc, (uint64_t)R * R, verts, normals, V, faces, t0, t1, flags, x, d, max_points, stream);
}

int cnerf_mesh_atlas_proj_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, const float *tangents, uint32_t t0, uint32_t t1, const float *m, uint32_t m_stride,
                                 const uint32_t *flags, float *rgb, uint32_t max_points, void *stream) {
    PjTexels loc;
    if (const int rc = pj_locate(V, F, R, ws, ws_bytes, loc)) return rc;
    return bake_launch_tspace(loc, (uint64_t)R * R, verts, normals, V, faces, tangents, t0, t1, m, m_stride, flags, rgb, max_points, stream);
}

int cnerf_mesh_atlas_proj_store(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, uint32_t t0, uint32_t t1, const float *rgb,
                                uint32_t rgb_stride, const uint32_t *flags, uint8_t *image, void *stream) {
    PjTexels loc;
    if (const int rc = pj_locate(V, F, R, ws, ws_bytes, loc)) return rc;
    static const uint8_t no_fill[3] = {0, 0, 0};             // never written: a listed texel has an owner
    return bake_launch_store(loc, (uint64_t)R * R, t0, t1, rgb, rgb_stride, no_fill, flags, image, stream);
}

int cnerf_mesh_atlas_proj_fill(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, const uint8_t *fill_host,
                               const uint32_t *flags, uint8_t *image, void *stream) {
    PjTexels loc;
    if (const int rc = pj_locate(V, F, R, ws, ws_bytes, loc)) return rc;
    if (!flags) return CNERF_ENULL;
    return bake_launch_fill(loc, fill_host, flags, image, stream);
}

}  // extern "C"
