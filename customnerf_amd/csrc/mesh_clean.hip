// Mesh cleanup on the device (cnerf_mesh_components_*, cnerf_mesh_cluster_*): removal of small connected components and simplification by
// vertex clustering, for any triangle mesh (marching-cubes output of mesh.hip or another).  Same conventions as mesh.hip: the caller's stream,
// caller-owned buffers and workspace, a count pass whose counts[3] = (vertices, faces, flags) are the only host read, then an emit pass.
// Output order never depends on scheduling: compaction is an exclusive scan of keep flags (mesh_common.h), and the only atomics are integer
// ones whose result does not depend on their order (min-root hooking, counts, 64-bit fixed-point sums, atomicMin).  NumPy restatement:
// tests/mesh_clean_restatement.py.  flags bit 0 (CC_BAD_INDEX): a face index outside [0, V); emit then writes nothing.
//
// Components (workspace: header | parent u32 [V] | face count u32 [V] | new index u32 [V] | workgroup totals uint2 [max(V, F) / 256]):
//   k_cc_init     : parent[v] = v, counts 0, flags 0
//   k_cc_hook     : per face, union of (f0, f1) and (f1, f2): lock-free union-find after ECL-CC (Jaiganesh & Burtscher 2018) — the larger
//                   root is hooked under the smaller one by atomicCAS, finds shorten the path they walk.  Parent indices only decrease.
//   k_cc_compress : parent[v] = root of v.  Every root is the smallest vertex of its tree, so the label of a component is its smallest vertex
//                   index, whatever order the CASes landed in.
//   k_cc_size     : faces per component, integer atomicAdd on the label of f0 (one per label and wave)
//   k_cc_largest  : one workgroup: the component with the most faces, the smaller label on a tie (max of (faces << 32 | ~label))
//   k_cc_count    : thread i: keep flag of vertex i and of face i; workgroup totals (ballot / popcount); then the shared one-workgroup scan
//   k_cc_verts / k_cc_faces : the workgroup prefix of the same flags -> new indices; faces remapped through them.  Input order is kept.
//
// Clustering (Lindstrom 2000, out-of-core simplification; workspace: header | vertex cell u32 [V] | occupancy u8 [G] | cluster of cell u32 [G]
//   | cell of cluster u32 [min(V, G)] | face hash u32 [H] | face slot u32 [F] | workgroup totals uint2 [max(G, F) / 256] | sums int64 [min(V, G)][16]):
//   k_cl_assign : cell of every vertex, clamp(floor((p - origin) / cell), 0, g - 1) per axis in float32; occupancy byte = 1
//   k_cl_hash   : per face whose three cells differ: insert its sorted cell triple into an open-addressing table of face indices; the slot of
//                 a triple ends up holding the smallest face index that has it (atomicCAS to claim, atomicMin on a match)
//   k_cl_count  : thread i: cell i occupied, face i the survivor of its slot; workgroup totals; the scan numbers clusters in linear cell order
//   k_cl_ids    : (emit) cluster id of every occupied cell, its cell, and its sums zeroed
//   k_cl_vsum   : per vertex: local position (relative to its cell's corner, in cell units), count and normal, added in fixed point
//   k_cl_fsum   : per face of nonzero area: its area-weighted plane quadric (A = a n n^T, b = a n d), in each distinct cluster's local frame
//   k_cl_solve  : per cluster in fp64: x = xbar + A+ (-b - A xbar), A+ from a 3x3 Jacobi eigen-solve without eigenvalues < 1e-3 lambda_max
//                 (mesh_qef.h), clamped to the cell; normal = normalised sum of the member normals
//   k_cl_faces  : survivors in input order, remapped to cluster ids in their input winding
//
// Fixed point (exact integer sums, order-independent: docs/HARDWARE_FACTS.md A.2; no float atomics).  Counts are < 2^31.
//   local positions u, scale 2^24: |u| < 2^7 for every vertex (a vertex inside the grid has u in [0, 1]) => |sum| < 2^31 * 2^7 * 2^24 = 2^62
//   normals, scale 2^28: |n_i| <= 1 (unit normals; any |n_i| < 8 is exact) => |sum| < 2^31 * 2^3 * 2^28 = 2^62
//   quadric entries, scale 2^32: a face of local area a (cell units) adds |a n_i n_j| <= a and |a n_i d| <= a |d|, d = -n . u0 in the
//     cluster's frame.  Exact while, per cluster, the sum over its faces of a * max(1, |d|) stays below 2^30 (about 10^9 cells^2) => |sum| < 2^62.
//     A marching-cubes face under cells of >= 2 lattice steps has a < 1 and |d| < 3; a cluster collects a few hundred of them.
#include "common.h"
#include "mesh_common.h"
#include "mesh_qef.h"

#define CC_BAD_INDEX 1u
#define CL_NONE 0xffffffffu
#define CL_SP 16777216.0                             // 2^24: local positions
#define CL_SN 268435456.0                            // 2^28: normals
#define CL_SQ 4294967296.0                           // 2^32: quadric entries
#define CL_ACC 16                                    // int64 per cluster: A00 A01 A02 A11 A12 A22 | b0 b1 b2 | u0 u1 u2 | n0 n1 n2 | count

namespace {

__device__ __forceinline__ void add_i64(int64_t *p, int64_t v) {
    if (v) __hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------ components
struct CcPtr {
    uint32_t *hdr;                                   // flags, largest label, its face count, kept vertices
    uint32_t *parent, *fcount, *remap;
    uint2 *sums;
    uint32_t n;                                      // threads of the count and emit passes: max(V, F), one workgroup at least
};

// the workspace: its regions in order -> total bytes (ws == nullptr: the size only)
uint64_t cc_carve(void *ws, uint32_t V, uint32_t F, CcPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.parent = c.take<uint32_t>(V);
    p.fcount = c.take<uint32_t>(V);
    p.remap = c.take<uint32_t>(V);
    p.n = V > F ? V : F;
    if (!p.n) p.n = 1;                               // also for an empty mesh
    p.sums = c.take<uint2>(cn_div_up64(p.n, MC_BLOCK));
    return c.total();
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_init(uint32_t V, uint32_t *__restrict__ parent, uint32_t *__restrict__ fcount,
                                                      uint32_t *__restrict__ hdr) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < V) {
        parent[i] = i;
        fcount[i] = 0;
    }
    if (i < 3) hdr[i] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_hook(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, uint32_t *parent,
                                                      uint32_t *__restrict__ hdr) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    if (!mesh_face(faces, f, V, t)) {
        atomicOr(hdr, CC_BAD_INDEX);
        return;
    }
    cc_union(parent, t[0], t[1]);
    cc_union(parent, t[1], t[2]);
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_compress(uint32_t V, uint32_t *parent) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    uint32_t r = ld_rlx(parent + v), n;
    while ((n = ld_rlx(parent + r)) != r) r = n;     // the forest is final: concurrent writers only store roots
    st_rlx(parent + v, r);
}

// Neighbouring faces mostly share a component: the lanes of a wave with one label add their count in one atomic (one per distinct label
// in the wave).  Adding 1 per face put every face of the largest component on one address: 18.9 ms for 1.7 M faces, against 2.1 ms for
// all of marching cubes at 512^3.
__global__ __launch_bounds__(MC_BLOCK) void k_cc_size(const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                      const uint32_t *__restrict__ label, uint32_t *__restrict__ fcount) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t t[3];
    const bool ok = f < F && mesh_face(faces, f, V, t);
    const uint32_t lab = ok ? label[t[0]] : CL_NONE;
    uint64_t todo = __ballot(ok);                    // wave-uniform
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t L = (uint32_t)__shfl((int)lab, leader);
        const uint64_t same = __ballot(ok && lab == L) & todo;
        if (cn_lane() == (uint32_t)leader) atomicAdd(fcount + L, (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_cc_largest(uint32_t V, const uint32_t *__restrict__ fcount, uint32_t *__restrict__ hdr) {
    __shared__ uint64_t red[MC_SCAN_BLOCK / CN_WAVE];
    uint64_t best = 0;
    for (uint32_t i = threadIdx.x; i < V; i += MC_SCAN_BLOCK) {
        const uint64_t key = ((uint64_t)fcount[i] << 32) | (uint64_t)(0xffffffffu - i);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = CN_WAVE / 2; o > 0; o >>= 1) {
        const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)best, o);
        best = x > best ? x : best;
    }
    if (cn_lane() == 0) red[threadIdx.x / CN_WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < MC_SCAN_BLOCK / CN_WAVE; ++j) best = red[j] > best ? red[j] : best;
        hdr[1] = 0xffffffffu - (uint32_t)best;
        hdr[2] = (uint32_t)(best >> 32);
    }
}

__device__ __forceinline__ bool cc_keep(uint32_t label, const uint32_t *__restrict__ fcount, uint32_t min_faces, int largest,
                                        const uint32_t *__restrict__ hdr) {
    const uint32_t n = fcount[label];
    return n >= min_faces && (!largest || (label == hdr[1] && n > 0));
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_count(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, const uint32_t *__restrict__ label,
                                                       const uint32_t *__restrict__ fcount, uint32_t min_faces, int largest,
                                                       const uint32_t *__restrict__ hdr, uint2 *__restrict__ sums) {
    __shared__ uint32_t red_v[MC_WAVES], red_f[MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t t[3];
    const uint32_t kv = i < V && cc_keep(label[i], fcount, min_faces, largest, hdr);
    const uint32_t kf = i < F && mesh_face(faces, i, V, t) && cc_keep(label[t[0]], fcount, min_faces, largest, hdr);
    const uint32_t tv = mc_block_total<1>(kv, red_v);
    const uint32_t tf = mc_block_total<1>(kf, red_f);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(tv, tf);
}

// one workgroup: the shared scan; counts = (kept vertices, kept faces, flags).  hdr[3] = kept vertices (clustering: clusters) for emit
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_clean_scan(uint2 *__restrict__ sums, uint32_t nblk, uint32_t *__restrict__ counts,
                                                              uint32_t *__restrict__ hdr) {
    uint64_t cv, cf;
    mc_scan_totals(sums, nblk, cv, cf);              // both <= max(V, F) or G, < 2^31
    if (threadIdx.x == 0) {
        counts[0] = (uint32_t)cv;
        counts[1] = (uint32_t)cf;
        counts[2] = hdr[0];
        hdr[3] = (uint32_t)cv;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_verts(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                       const uint32_t *__restrict__ label, const uint32_t *__restrict__ fcount, uint32_t min_faces,
                                                       int largest, const uint32_t *__restrict__ hdr, const uint2 *__restrict__ sums,
                                                       uint32_t *__restrict__ remap, float *__restrict__ verts_out, float *__restrict__ normals_out,
                                                       int32_t *__restrict__ old_index, uint32_t max_verts) {
    __shared__ uint32_t red[MC_WAVES];
    if (hdr[0]) return;                              // a bad face index: nothing is written
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t kv = i < V && cc_keep(label[i], fcount, min_faces, largest, hdr);
    const uint32_t k = sums[blockIdx.x].x + mc_block_prefix<1>(kv, red);
    if (i >= V) return;
    remap[i] = kv ? k : CL_NONE;
    if (kv) mesh_emit_vertex(verts, normals, i, k, verts_out, normals_out, old_index, max_verts);
}

__global__ __launch_bounds__(MC_BLOCK) void k_cc_faces(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, const uint32_t *__restrict__ label,
                                                       const uint32_t *__restrict__ fcount, uint32_t min_faces, int largest,
                                                       const uint32_t *__restrict__ hdr, const uint2 *__restrict__ sums,
                                                       const uint32_t *__restrict__ remap, int32_t *__restrict__ faces_out, uint32_t max_faces) {
    __shared__ uint32_t red[MC_WAVES];
    if (hdr[0]) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t t[3];
    const uint32_t kf = i < F && mesh_face(faces, i, V, t) && cc_keep(label[t[0]], fcount, min_faces, largest, hdr);
    const uint32_t k = sums[blockIdx.x].y + mc_block_prefix<1>(kf, red);
    if (!kf || k >= max_faces) return;
    const uint64_t d = 3 * (uint64_t)k;
#pragma unroll
    for (int q = 0; q < 3; ++q) faces_out[d + q] = (int32_t)remap[t[q]];
}

int cc_check_dims(uint32_t V, uint32_t F) { return (V >= (1u << 31) || F >= (1u << 31)) ? CNERF_EINVAL : CNERF_OK; }

// ------------------------------------------------------------------------------------------------ clustering
struct ClGeom {
    float org[3], cell[3], gm1f[3];
    uint32_t g[3];
};

struct ClPtr {
    uint32_t *hdr;                                   // flags, -, -, cluster count
    uint32_t *vcell;
    uint8_t *occ;
    uint32_t *cid, *ccell, *table, *fslot;
    uint2 *sums;
    int64_t *acc;
    uint64_t H;                                      // slots of the face hash
    uint32_t n;                                      // threads of the count and emit passes: max(G, F)
};

// the workspace: its regions in order -> total bytes (ws == nullptr: the size only)
uint64_t cl_carve(void *ws, uint64_t V, uint64_t F, uint64_t G, ClPtr &p) {
    p.H = 64;
    while (p.H < 2 * F) p.H <<= 1;                   // load factor <= 1/2; F < 2^31 => H <= 2^32, slot indices fit a uint32 mask
    const uint64_t K = V < G ? V : G;
    p.n = (uint32_t)(G > F ? G : F);
    MeshCarve c(ws);
    p.hdr = c.header();
    p.vcell = c.take<uint32_t>(V);
    p.occ = c.take<uint8_t>(G);
    p.cid = c.take<uint32_t>(G);
    p.ccell = c.take<uint32_t>(K);
    p.table = c.take<uint32_t>(p.H);
    p.fslot = c.take<uint32_t>(F);
    p.sums = c.take<uint2>(cn_div_up64(p.n, MC_BLOCK));
    p.acc = c.take<int64_t>(CL_ACC * K);
    return c.total();
}

__device__ __forceinline__ uint32_t cl_cell(const float *__restrict__ verts, uint32_t v, const ClGeom &g, uint32_t c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = (verts[3 * (uint64_t)v + a] - g.org[a]) / g.cell[a];
        const float f = fminf(fmaxf(floorf(q), 0.0f), g.gm1f[a]);      // NaN -> 0
        const uint32_t ci = (uint32_t)f;
        c[a] = ci < g.g[a] - 1 ? ci : g.g[a] - 1;    // (float)(g - 1) may round up
    }
    return (c[0] * g.g[1] + c[1]) * g.g[2] + c[2];   // < 2^31
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_assign(const float *__restrict__ verts, uint32_t V, ClGeom g, uint32_t *__restrict__ vcell,
                                                        uint8_t *__restrict__ occ) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    uint32_t c[3];
    const uint32_t lin = cl_cell(verts, v, g, c);
    vcell[v] = lin;
    occ[lin] = 1;
}

__device__ __forceinline__ void sort3(uint32_t &a, uint32_t &b, uint32_t &c) {
    uint32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// sorted cell triple of a valid face, false when two cells are equal
__device__ __forceinline__ bool cl_key(const int32_t *__restrict__ faces, uint32_t f, const uint32_t *__restrict__ vcell, uint32_t k[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) k[q] = vcell[faces[3 * (uint64_t)f + q]];
    sort3(k[0], k[1], k[2]);
    return k[0] != k[1] && k[1] != k[2];
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_hash(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, const uint32_t *__restrict__ vcell,
                                                      uint32_t *table, uint32_t hmask, uint32_t *__restrict__ fslot, uint32_t *__restrict__ hdr) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3], k[3];
    if (!mesh_face(faces, f, V, t)) {
        atomicOr(hdr, CC_BAD_INDEX);
        fslot[f] = CL_NONE;
        return;
    }
    if (!cl_key(faces, f, vcell, k)) {
        fslot[f] = CL_NONE;                          // collapses into an edge or a point
        return;
    }
    uint64_t h = (uint64_t)k[0] * 0x9E3779B97F4A7C15ull ^ (uint64_t)k[1] * 0xC2B2AE3D27D4EB4Full ^ (uint64_t)k[2] * 0x165667B19E3779F9ull;
    h ^= h >> 31;
    uint32_t s = (uint32_t)h & hmask;
    for (;;) {                                       // H > 2 * (inserted triples): an empty slot is always ahead
        uint32_t cur = ld_rlx(table + s);
        if (cur == CL_NONE) {
            cur = atomicCAS(table + s, CL_NONE, f);
            if (cur == CL_NONE) break;               // claimed
        }
        uint32_t k2[3];
        cl_key(faces, cur, vcell, k2);               // cur only ever changes to a face with the same triple
        if (k2[0] == k[0] && k2[1] == k[1] && k2[2] == k[2]) {
            atomicMin(table + s, f);
            break;
        }
        s = (s + 1) & hmask;
    }
    fslot[f] = s;
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_count(uint32_t G, uint32_t F, const uint8_t *__restrict__ occ, const uint32_t *__restrict__ table,
                                                       const uint32_t *__restrict__ fslot, uint2 *__restrict__ sums) {
    __shared__ uint32_t red_v[MC_WAVES], red_f[MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t kc = i < G && occ[i];
    uint32_t kf = 0;
    if (i < F) {
        const uint32_t s = fslot[i];
        kf = s != CL_NONE && table[s] == i;
    }
    const uint32_t tc = mc_block_total<1>(kc, red_v);
    const uint32_t tf = mc_block_total<1>(kf, red_f);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(tc, tf);
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_ids(uint32_t G, const uint8_t *__restrict__ occ, const uint2 *__restrict__ sums,
                                                     const uint32_t *__restrict__ hdr, uint32_t *__restrict__ cid, uint32_t *__restrict__ ccell,
                                                     int64_t *__restrict__ acc) {
    __shared__ uint32_t red[MC_WAVES];
    if (hdr[0]) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t kc = i < G && occ[i];
    const uint32_t k = sums[blockIdx.x].x + mc_block_prefix<1>(kc, red);
    if (!kc) return;
    cid[i] = k;
    ccell[k] = i;
    longlong2 *a = (longlong2 *)(acc + CL_ACC * (uint64_t)k);
#pragma unroll
    for (int q = 0; q < CL_ACC / 2; ++q) a[q] = make_longlong2(0, 0);
}

// corner of cluster cell `lin` (linear index) in world units, fp64
__device__ __forceinline__ void cl_corner(uint32_t lin, const ClGeom &g, double o[3]) {
    const uint32_t cz = lin % g.g[2], r = lin / g.g[2], cy = r % g.g[1], cx = r / g.g[1];
    const uint32_t c[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (double)g.org[a] + (double)g.cell[a] * (double)c[a];
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_vsum(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V, ClGeom g,
                                                      const uint32_t *__restrict__ vcell, const uint32_t *__restrict__ cid,
                                                      const uint32_t *__restrict__ hdr, int64_t *__restrict__ acc) {
    if (hdr[0]) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const uint32_t lin = vcell[v];
    int64_t *a = acc + CL_ACC * (uint64_t)cid[lin];
    double o[3];
    cl_corner(lin, g, o);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double u = ((double)verts[3 * (uint64_t)v + q] - o[q]) / (double)g.cell[q];
        add_i64(a + 9 + q, u == u ? __double2ll_rn(u * CL_SP) : 0);
        if (normals) {
            const double n = (double)normals[3 * (uint64_t)v + q];
            add_i64(a + 12 + q, n == n ? __double2ll_rn(n * CL_SN) : 0);
        }
    }
    add_i64(a + 15, 1);
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_fsum(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                      ClGeom g, const uint32_t *__restrict__ vcell, const uint32_t *__restrict__ cid,
                                                      const uint32_t *__restrict__ hdr, int64_t *__restrict__ acc) {
    if (hdr[0]) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t t[3];
    if (f >= F || !mesh_face(faces, f, V, t)) return;
    double p[3][3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[q][a] = (double)verts[3 * (uint64_t)t[q] + a];
    double e1[3], e2[3];                             // edges in cell units (the local frames differ by a translation only)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = (p[1][a] - p[0][a]) / (double)g.cell[a];
        e2[a] = (p[2][a] - p[0][a]) / (double)g.cell[a];
    }
    const double m[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double mm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    if (!(mm > 0.0) || !(mm < 1e300)) return;        // zero area or non-finite: no plane
    const double n[3] = {m[0] / mm, m[1] / mm, m[2] / mm}, area = 0.5 * mm;
    const double A[6] = {area * n[0] * n[0], area * n[0] * n[1], area * n[0] * n[2], area * n[1] * n[1], area * n[1] * n[2], area * n[2] * n[2]};
    int64_t qa[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) qa[j] = __double2ll_rn(A[j] * CL_SQ);
    uint32_t cells[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) cells[q] = vcell[t[q]];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if ((q > 0 && cells[q] == cells[0]) || (q > 1 && cells[q] == cells[1])) continue;     // once per distinct cluster
        double o[3];
        cl_corner(cells[q], g, o);
        double d = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) d -= n[a] * ((p[0][a] - o[a]) / (double)g.cell[a]);
        int64_t *ac = acc + CL_ACC * (uint64_t)cid[cells[q]];
#pragma unroll
        for (int j = 0; j < 6; ++j) add_i64(ac + j, qa[j]);
#pragma unroll
        for (int a = 0; a < 3; ++a) add_i64(ac + 6 + a, __double2ll_rn(area * n[a] * d * CL_SQ));
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_solve(ClGeom g, const uint32_t *__restrict__ ccell, const int64_t *__restrict__ acc,
                                                       const uint32_t *__restrict__ hdr, int has_normals, float *__restrict__ verts_out,
                                                       float *__restrict__ normals_out, uint32_t max_verts) {
    if (hdr[0]) return;
    const uint32_t k = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (k >= hdr[3] || k >= max_verts) return;
    const int64_t *a = acc + CL_ACC * (uint64_t)k;
    const double cnt = (double)a[15];
    double s[6], b[3], xb[3];
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = (double)a[j] / CL_SQ;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        b[j] = (double)a[6 + j] / CL_SQ;
        xb[j] = (double)a[9 + j] / CL_SP / cnt;
    }
    double x[3];
    qef_solve(s, b, xb, x);
    double o[3];
    cl_corner(ccell[k], g, o);
    const uint64_t d = 3 * (uint64_t)k;
#pragma unroll
    for (int j = 0; j < 3; ++j) verts_out[d + j] = (float)(o[j] + fmin(fmax(x[j], 0.0), 1.0) * (double)g.cell[j]);
    if (has_normals && normals_out) {
        const double n[3] = {(double)a[12] / CL_SN, (double)a[13] / CL_SN, (double)a[14] / CL_SN};
        const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) normals_out[d + j] = l > 0.0 ? (float)(n[j] / l) : 0.0f;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_cl_faces(const int32_t *__restrict__ faces, uint32_t F, const uint32_t *__restrict__ table,
                                                       const uint32_t *__restrict__ fslot, const uint32_t *__restrict__ vcell,
                                                       const uint32_t *__restrict__ cid, const uint32_t *__restrict__ hdr,
                                                       const uint2 *__restrict__ sums, int32_t *__restrict__ faces_out, uint32_t max_faces) {
    __shared__ uint32_t red[MC_WAVES];
    if (hdr[0]) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t kf = 0;
    if (i < F) {
        const uint32_t s = fslot[i];
        kf = s != CL_NONE && table[s] == i;
    }
    const uint32_t k = sums[blockIdx.x].y + mc_block_prefix<1>(kf, red);
    if (!kf || k >= max_faces) return;
    const uint64_t d = 3 * (uint64_t)k;
#pragma unroll
    for (int q = 0; q < 3; ++q) faces_out[d + q] = (int32_t)cid[vcell[faces[3 * (uint64_t)i + q]]];
}

int cl_check(uint32_t V, uint32_t F, const uint32_t *grid_host, uint64_t *G) {
    if (const int rc = cc_check_dims(V, F)) return rc;
    if (!grid_host) return CNERF_ENULL;
    if (!grid_host[0] || !grid_host[1] || !grid_host[2]) return CNERF_EINVAL;
    *G = (uint64_t)grid_host[0] * grid_host[1] * grid_host[2];
    return *G >= (1ull << 31) ? CNERF_EINVAL : CNERF_OK;
}

int cl_geom(const float *origin_host, const float *cell_host, const uint32_t *grid_host, ClGeom *g) {
    for (int a = 0; a < 3; ++a) {
        const float o = origin_host[a], c = cell_host[a];
        if (!(o == o && o - o == 0.0f) || !(c > 0.0f && c - c == 0.0f)) return CNERF_EINVAL;     // finite origin, finite cell > 0
        g->org[a] = o;
        g->cell[a] = c;
        g->g[a] = grid_host[a];
        g->gm1f[a] = (float)(grid_host[a] - 1);
    }
    return CNERF_OK;
}

int cn_memset(void *p, int v, uint64_t n, void *stream) {
    return n ? (int)hipMemsetAsync(p, v, n, CN_STREAM(stream)) : 0;
}

}  // namespace

extern "C" {

int cnerf_mesh_components_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (const int rc = cc_check_dims(V, F)) return rc;
    if (!bytes_host) return CNERF_ENULL;
    CcPtr p;
    *bytes_host = cc_carve(nullptr, V, F, p);
    return CNERF_OK;
}

int cnerf_mesh_components_count(const int32_t *faces, uint32_t V, uint32_t F, uint32_t min_faces, int largest, void *ws, uint64_t ws_bytes,
                                uint32_t *counts, void *stream) {
    if (const int rc = cc_check_dims(V, F)) return rc;
    if ((F && !faces) || !ws || !counts) return CNERF_ENULL;
    CcPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, cc_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    hipLaunchKernelGGL(k_cc_init, mesh_grid(V ? V : 1), dim3(MC_BLOCK), 0, st, V, p.parent, p.fcount, p.hdr);
    if (F) {
        hipLaunchKernelGGL(k_cc_hook, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, p.parent, p.hdr);
        if (V) hipLaunchKernelGGL(k_cc_compress, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p.parent);
        hipLaunchKernelGGL(k_cc_size, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, (const uint32_t *)p.parent, p.fcount);
    }
    if (largest) hipLaunchKernelGGL(k_cc_largest, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, V, (const uint32_t *)p.fcount, p.hdr);
    hipLaunchKernelGGL(k_cc_count, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, faces, V, F, (const uint32_t *)p.parent, (const uint32_t *)p.fcount,
                       min_faces, largest, (const uint32_t *)p.hdr, p.sums);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, p.sums, cn_div_up(p.n, MC_BLOCK), counts, p.hdr);
    return cn_launch_status();
}

int cnerf_mesh_components_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t min_faces,
                               int largest, void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out, int32_t *faces_out,
                               int32_t *old_index, uint32_t max_verts, uint32_t max_faces, void *stream) {
    if (const int rc = cc_check_dims(V, F)) return rc;
    if ((V && !verts) || (F && !faces) || !ws || (max_verts && !verts_out) || (max_faces && !faces_out)) return CNERF_ENULL;
    CcPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, cc_carve(ws, V, F, p))) return rc;
    const uint32_t *hdr = p.hdr, *label = p.parent, *fcount = p.fcount;
    const uint2 *sums = p.sums;
    hipStream_t st = CN_STREAM(stream);
    hipLaunchKernelGGL(k_cc_verts, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, verts, normals, V, label, fcount, min_faces, largest, hdr, sums,
                       p.remap, verts_out, max_verts ? normals_out : nullptr, max_verts ? old_index : nullptr, max_verts);
    hipLaunchKernelGGL(k_cc_faces, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, faces, V, F, label, fcount, min_faces, largest, hdr, sums,
                       (const uint32_t *)p.remap, faces_out, max_faces);
    return cn_launch_status();
}

int cnerf_mesh_cluster_workspace_bytes(uint32_t V, uint32_t F, const uint32_t *grid_host, uint64_t *bytes_host) {
    uint64_t G;
    if (const int rc = cl_check(V, F, grid_host, &G)) return rc;
    if (!bytes_host) return CNERF_ENULL;
    ClPtr p;
    *bytes_host = cl_carve(nullptr, V, F, G, p);
    return CNERF_OK;
}

int cnerf_mesh_cluster_count(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, const float *origin_host, const float *cell_host,
                             const uint32_t *grid_host, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream) {
    uint64_t G;
    if (const int rc = cl_check(V, F, grid_host, &G)) return rc;
    if ((V && !verts) || (F && !faces) || !origin_host || !cell_host || !ws || !counts) return CNERF_ENULL;
    ClGeom g;
    if (const int rc = cl_geom(origin_host, cell_host, grid_host, &g)) return rc;
    ClPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, cl_carve(ws, V, F, G, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    int rc = cn_memset(p.hdr, 0, 256, stream);
    if (!rc) rc = cn_memset(p.occ, 0, G, stream);
    if (!rc) rc = cn_memset(p.table, 0xff, 4ull * p.H, stream);
    if (rc) return rc;
    if (V) hipLaunchKernelGGL(k_cl_assign, mesh_grid(V), dim3(MC_BLOCK), 0, st, verts, V, g, p.vcell, p.occ);
    if (F) hipLaunchKernelGGL(k_cl_hash, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, (const uint32_t *)p.vcell, p.table, (uint32_t)(p.H - 1),
                              p.fslot, p.hdr);
    hipLaunchKernelGGL(k_cl_count, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, (uint32_t)G, F, (const uint8_t *)p.occ, (const uint32_t *)p.table,
                       (const uint32_t *)p.fslot, p.sums);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, p.sums, cn_div_up(p.n, MC_BLOCK), counts, p.hdr);
    return cn_launch_status();
}

int cnerf_mesh_cluster_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, const float *origin_host,
                            const float *cell_host, const uint32_t *grid_host, void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out,
                            int32_t *faces_out, uint32_t max_verts, uint32_t max_faces, void *stream) {
    uint64_t G;
    if (const int rc = cl_check(V, F, grid_host, &G)) return rc;
    if ((V && !verts) || (F && !faces) || !origin_host || !cell_host || !ws || (max_verts && !verts_out) || (max_faces && !faces_out))
        return CNERF_ENULL;
    ClGeom g;
    if (const int rc = cl_geom(origin_host, cell_host, grid_host, &g)) return rc;
    ClPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, cl_carve(ws, V, F, G, p))) return rc;
    const uint32_t *hdr = p.hdr, *vcell = p.vcell, *cid = p.cid, *table = p.table, *fslot = p.fslot;
    const uint2 *sums = p.sums;
    hipStream_t st = CN_STREAM(stream);
    hipLaunchKernelGGL(k_cl_ids, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, (uint32_t)G, (const uint8_t *)p.occ, sums, hdr, p.cid, p.ccell, p.acc);
    if (V) hipLaunchKernelGGL(k_cl_vsum, mesh_grid(V), dim3(MC_BLOCK), 0, st, verts, normals, V, g, vcell, cid, hdr, p.acc);
    if (F) hipLaunchKernelGGL(k_cl_fsum, mesh_grid(F), dim3(MC_BLOCK), 0, st, verts, faces, V, F, g, vcell, cid, hdr, p.acc);
    if (max_verts)
        hipLaunchKernelGGL(k_cl_solve, mesh_grid(max_verts), dim3(MC_BLOCK), 0, st, g, (const uint32_t *)p.ccell, (const int64_t *)p.acc, hdr,
                           normals ? 1 : 0, verts_out, normals_out, max_verts);
    hipLaunchKernelGGL(k_cl_faces, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, faces, F, table, fslot, vcell, cid, hdr, sums, faces_out, max_faces);
    return cn_launch_status();
}

}  // extern "C"
