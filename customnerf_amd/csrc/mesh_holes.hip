// Mesh topology report and boundary-loop hole filling on the device (cnerf_mesh_topology*, cnerf_mesh_holes_*).  Same conventions as
// mesh_clean.hip: the caller's stream, caller-owned buffers and workspace, a count pass whose small counts array is the only host read,
// then an emit pass.  Output never depends on scheduling: compaction is an exclusive scan of flags (mesh_common.h), the lists are sorted,
// and the only atomics are integer ones whose result does not depend on their order (degrees, list slots before the sort, min-root
// hooking, loop lengths, flag bits).  The rules are in include/customnerf_hip.h; NumPy restatement: tests/holes_restatement.py.
//
// Half-edge h = 3 f + k runs from a = f[k] to b = f[(k + 1) % 3]; a == b (a face repeating an index) is no edge.  Both passes share one
// analysis (workspace: header | per vertex: degree, list end, component parent, a boundary half-edge u32 [V], marks u8 [V] | per
// half-edge: list, loop parent, loop length, next u32 [3 F], class u8 [3 F] | workgroup totals u32 [max(V, 3 F) / 256][9]):
//   k_ho_clear   : degrees 0, parents = self, lengths 0, next = none, flags 0
//   k_ho_load    : per face: the index check, the repeated-index flag, degrees (atomicAdd), vertex components (topology: cc_union)
//   k_ho_vsum / k_ho_scan / k_ho_offsets / k_ho_fill / k_ho_sort : one CSR of outgoing half-edges per start vertex, each list in
//                  increasing half-edge id (slots by atomicAdd, then sorted)
//   k_ho_class   : per half-edge a -> b: same = the half-edges a -> b (itself included), opp = the half-edges b -> a, from the two lists:
//                  interior (1 and 1), boundary (1 in all), else non-manifold; canonical when it is the smallest id of them all, which
//                  is what counts undirected edges once
//   k_ho_vertex  : per vertex, over its corners: outgoing and incoming boundary half-edges; more than one of either: pinched; all of
//                  them joined in the loop union-find (root = smallest half-edge id = the loop's label); one of each: next[in] = out
//   k_ho_loops   : loop parents compressed to roots, lengths added at the root (one atomic per root and wave: see k_cc_size of
//                  mesh_clean.hip on one-address hot spots), loops through a pinched vertex or an end of a non-manifold edge marked open
//   count        : thread i looks at vertex i, half-edge i and face i; workgroup totals of the counters, then the shared one-workgroup scan
//   emit         : the workgroup prefix of the same flags -> slots.  Filling: thread h of a filled loop's label walks next from h:
//                  faces (b, a, c) in loop order, the centroid summed in fp64 in loop order and rounded once, then the normal from the
//                  fan's cross products in fp64 in loop order.  The walk is serial per loop (a chain of n dependent loads).
#include "common.h"
#include "mesh_common.h"

#define HO_BAD_INDEX 1u
#define HO_NON_MANIFOLD 2u
#define HO_REPEATED 4u
#define HO_NONE 0xffffffffu
#define HO_MAX_F 0x2aaaaaaau                         // half-edge ids 3 f + k and loop lengths stay below 2^31
#define HO_INTERIOR 1u                               // class byte: low two bits the kind (0: no edge) ...
#define HO_BOUNDARY 2u
#define HO_NONMAN 3u
#define HO_KIND 3u
#define HO_CANON 4u                                  // ... bit 2: the smallest half-edge id on its undirected edge
#define HO_OPEN 0x80000000u                          // length word of a loop's root: the loop is not simple
#define HO_LEN 0x7fffffffu
#define HO_NT 9                                      // counters of the topology report
#define HO_NF 5                                      // counters of the fill pass
#define HO_V_PINCHED 1u
#define HO_V_NONMAN 2u

namespace {

struct HoPtr {
    uint32_t *hdr;                                   // flags
    uint32_t *deg, *end, *vparent, *vfb;
    uint8_t *vfl;
    uint32_t *list, *parent, *len, *nxt;
    uint8_t *cls;
    uint32_t *sums;
    uint32_t n;                                      // threads of the count and emit passes: max(V, 3 F), one at least
};

// the workspace: its regions in order -> total bytes (ws == nullptr: the size only)
uint64_t ho_carve(void *ws, uint64_t V, uint64_t F, HoPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.deg = c.take<uint32_t>(V);
    p.end = c.take<uint32_t>(V);
    p.vparent = c.take<uint32_t>(V);
    p.vfb = c.take<uint32_t>(V);
    p.vfl = c.take<uint8_t>(V);
    p.list = c.take<uint32_t>(3 * F);
    p.parent = c.take<uint32_t>(3 * F);
    p.len = c.take<uint32_t>(3 * F);
    p.nxt = c.take<uint32_t>(3 * F);
    p.cls = c.take<uint8_t>(3 * F);
    const uint64_t n = V > 3 * F ? V : 3 * F;
    p.n = (uint32_t)(n ? n : 1);
    p.sums = c.take<uint32_t>(HO_NT * cn_div_up64(p.n, MC_BLOCK));     // (also the uint2 totals of the list offsets)
    return c.total();
}

__device__ __forceinline__ uint32_t ho_next(uint32_t k) { return k == 2 ? 0 : k + 1; }
__device__ __forceinline__ uint32_t ho_from(const int32_t *__restrict__ fa, uint32_t h) { return (uint32_t)fa[h]; }
__device__ __forceinline__ uint32_t ho_to(const int32_t *__restrict__ fa, uint32_t h) {
    const uint32_t f = h / 3, k = h - 3 * f;
    return mesh_fv(fa, f, ho_next(k));
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_clear(uint32_t V, uint32_t F3, HoPtr p) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < V) {
        p.deg[i] = 0;
        p.vparent[i] = i;
    }
    if (i < F3) {
        p.parent[i] = i;
        p.len[i] = 0;
        p.nxt[i] = HO_NONE;
    }
    if (i < 64) p.hdr[i] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_load(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, int want_cc, HoPtr p) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    if (!mesh_face(faces, f, V, t)) {
        atomicOr(p.hdr, HO_BAD_INDEX);
        return;
    }
    if ((t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) && !(ld_rlx(p.hdr) & HO_REPEATED)) atomicOr(p.hdr, HO_REPEATED);
#pragma unroll
    for (int q = 0; q < 3; ++q) atomicAdd(p.deg + t[q], 1u);
    if (want_cc) {
        cc_union(p.vparent, t[0], t[1]);
        cc_union(p.vparent, t[1], t[2]);
    }
}

// workgroup totals of (degree, referenced)
__global__ __launch_bounds__(MC_BLOCK) void k_ho_vsum(uint32_t V, HoPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t d = v < V ? p.deg[v] : 0;
    mesh_csr_totals(d, d ? 1u : 0u, (uint2 *)p.sums);
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_ho_scan(uint32_t nblk, HoPtr p) {
    uint64_t cx, cy;
    mc_scan_totals((uint2 *)p.sums, nblk, cx, cy);   // sum of degrees <= 3 F < 2^31
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_offsets(uint32_t V, HoPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t start = mesh_csr_start(((const uint2 *)p.sums)[blockIdx.x].x, v < V ? p.deg[v] : 0, red);
    if (v < V) p.end[v] = start;                     // k_ho_fill advances it to start + degree
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_fill(const int32_t *__restrict__ fa, uint32_t F, HoPtr p) {
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) p.list[atomicAdd(p.end + mesh_fv(fa, f, q), 1u)] = 3 * f + q;
}

// each vertex sorts its own list; the component forest is final: parent[v] = root of v
__global__ __launch_bounds__(MC_BLOCK) void k_ho_sort(uint32_t V, int want_cc, HoPtr p) {
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    mesh_isort(p.list + (p.end[v] - p.deg[v]), p.deg[v]);
    if (want_cc) {
        uint32_t r = ld_rlx(p.vparent + v), n;
        while ((n = ld_rlx(p.vparent + r)) != r) r = n;
        st_rlx(p.vparent + v, r);
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_class(const int32_t *__restrict__ fa, uint32_t F3, HoPtr p) {
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t h = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (h >= F3) return;
    const uint32_t a = ho_from(fa, h), b = ho_to(fa, h);
    if (a == b) {
        p.cls[h] = 0;
        return;
    }
    uint32_t same = 0, opp = 0, lo = h;
    for (uint32_t i = p.end[a] - p.deg[a]; i < p.end[a]; ++i) {
        const uint32_t g = p.list[i];
        if (ho_to(fa, g) == b) {
            ++same;
            lo = g < lo ? g : lo;
        }
    }
    for (uint32_t i = p.end[b] - p.deg[b]; i < p.end[b]; ++i) {
        const uint32_t g = p.list[i];
        if (ho_to(fa, g) == a) {
            ++opp;
            lo = g < lo ? g : lo;
        }
    }
    const uint32_t kind = (same == 1 && opp == 1) ? HO_INTERIOR : (same + opp == 1) ? HO_BOUNDARY : HO_NONMAN;
    p.cls[h] = (uint8_t)(kind | (lo == h ? HO_CANON : 0u));
    if (kind == HO_NONMAN && !(ld_rlx(p.hdr) & HO_NON_MANIFOLD)) atomicOr(p.hdr, HO_NON_MANIFOLD);
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_vertex(uint32_t V, HoPtr p) {
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    uint32_t n_out = 0, n_in = 0, nm = 0, first = HO_NONE, h_out = HO_NONE, h_in = HO_NONE;
    for (uint32_t i = p.end[v] - p.deg[v]; i < p.end[v]; ++i) {
        const uint32_t h = p.list[i], f = h / 3, k = h - 3 * f;
        const uint32_t hin = 3 * f + (k == 0 ? 2 : k - 1);       // the half-edge of the same corner that ends in v
        const uint32_t pair[2] = {h, hin};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint32_t kind = p.cls[pair[q]] & HO_KIND;
            nm |= kind == HO_NONMAN;
            if (kind != HO_BOUNDARY) continue;
            if (q == 0) {
                ++n_out;
                h_out = h;
            } else {
                ++n_in;
                h_in = hin;
            }
            if (first == HO_NONE) first = pair[q];
            else cc_union(p.parent, first, pair[q]);
        }
    }
    if (n_out == 1 && n_in == 1) p.nxt[h_in] = h_out;
    p.vfb[v] = first;
    p.vfl[v] = (uint8_t)(((n_out > 1 || n_in > 1) ? HO_V_PINCHED : 0u) | (nm ? HO_V_NONMAN : 0u));
}

// the forests are final: concurrent writers only store roots
__device__ __forceinline__ uint32_t ho_root(const uint32_t *parent, uint32_t x) {
    uint32_t r = ld_rlx(parent + x), n;
    while ((n = ld_rlx(parent + r)) != r) r = n;
    return r;
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_loops(uint32_t V, uint32_t F3, HoPtr p) {
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool bnd = i < F3 && (p.cls[i] & HO_KIND) == HO_BOUNDARY;
    uint32_t root = HO_NONE;
    if (bnd) {
        root = ho_root(p.parent, i);
        st_rlx(p.parent + i, root);
    }
    uint64_t todo = __ballot(bnd);                   // wave-uniform: one add per distinct root in the wave
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t L = (uint32_t)__shfl((int)root, leader);
        const uint64_t same = __ballot(bnd && root == L) & todo;
        if (cn_lane() == (uint32_t)leader) atomicAdd(p.len + L, (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if (i < V && p.vfl[i] && p.vfb[i] != HO_NONE) atomicOr(p.len + ho_root(p.parent, p.vfb[i]), HO_OPEN);
}

// the analysis both passes share; the workspace then describes the mesh
void ho_analyse(const int32_t *faces, uint32_t V, uint32_t F, int want_cc, const HoPtr &p, hipStream_t st) {
    const uint32_t F3 = 3 * F, Vg = V ? V : 1;
    hipLaunchKernelGGL(k_ho_clear, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, V, F3, p);
    hipLaunchKernelGGL(k_ho_load, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, want_cc, p);
    hipLaunchKernelGGL(k_ho_vsum, mesh_grid(Vg), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_ho_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (uint32_t)cn_div_up64(Vg, MC_BLOCK), p);
    hipLaunchKernelGGL(k_ho_offsets, mesh_grid(Vg), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_ho_fill, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, F, p);
    hipLaunchKernelGGL(k_ho_sort, mesh_grid(Vg), dim3(MC_BLOCK), 0, st, V, want_cc, p);
    hipLaunchKernelGGL(k_ho_class, mesh_grid(F3), dim3(MC_BLOCK), 0, st, faces, F3, p);
    hipLaunchKernelGGL(k_ho_vertex, mesh_grid(Vg), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_ho_loops, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, V, F3, p);
}

// half-edge h is the label of a boundary loop
__device__ __forceinline__ bool ho_is_loop(uint32_t h, uint32_t F3, const HoPtr &p) {
    return h < F3 && (p.cls[h] & HO_KIND) == HO_BOUNDARY && p.parent[h] == h;
}

// ------------------------------------------------------------------------------------------------ topology
__global__ __launch_bounds__(MC_BLOCK) void k_ho_tcount(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, HoPtr p) {
    __shared__ uint32_t red[HO_NT][MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x, F3 = 3 * F;
    const bool ok = !(p.hdr[0] & HO_BAD_INDEX);      // uniform over the grid
    uint32_t c[HO_NT] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok && i < V) {
        c[0] = p.deg[i] > 0;                         // vertices used
        c[4] = (p.vfl[i] & HO_V_PINCHED) != 0;
        c[7] = c[0] && p.vparent[i] == i;            // components that hold a face
    }
    if (ok && i < F3) {
        const uint32_t cl = p.cls[i], kind = cl & HO_KIND;
        c[1] = (cl & HO_CANON) != 0;                 // undirected edges
        c[2] = kind == HO_BOUNDARY;
        c[3] = c[1] && kind == HO_NONMAN;
        c[5] = ho_is_loop(i, F3, p);
        c[6] = c[5] && !(p.len[i] & HO_OPEN);
    }
    uint32_t t[3];
    if (ok && i < F && mesh_face(faces, i, V, t)) c[8] = t[0] == t[1] || t[1] == t[2] || t[0] == t[2];
#pragma unroll
    for (int q = 0; q < HO_NT; ++q) {
        const uint32_t tot = mc_block_total<1>(c[q], red[q]);
        if (threadIdx.x == 0) p.sums[(uint64_t)blockIdx.x * HO_NT + q] = tot;
    }
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_ho_tscan(uint32_t nblk, HoPtr p, uint32_t *__restrict__ counts) {
    uint64_t tot[HO_NT];
    mc_scan_totals_n<HO_NT>(p.sums, nblk, tot);      // every total <= max(V, 3 F) < 2^31
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < HO_NT; ++q) counts[q] = (uint32_t)tot[q];
        counts[HO_NT] = p.hdr[0];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_tloops(uint32_t F3, HoPtr p, int32_t *__restrict__ loop_lengths, uint32_t max_loops) {
    __shared__ uint32_t red[MC_WAVES];
    if (p.hdr[0] & HO_BAD_INDEX) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t is = ho_is_loop(i, F3, p);
    const uint32_t k = p.sums[(uint64_t)blockIdx.x * HO_NT + 5] + mc_block_prefix<1>(is, red);
    if (is && k < max_loops) loop_lengths[k] = (int32_t)(p.len[i] & HO_LEN);
}

// ------------------------------------------------------------------------------------------------ hole filling
// edges of the loop labelled h when it is filled, else 0; *kind (when given): 1 a loop left open as not simple, 2 as too long
__device__ __forceinline__ uint32_t ho_fill_len(uint32_t h, uint32_t F3, uint32_t max_edges, const HoPtr &p, uint32_t *kind) {
    if (kind) *kind = 0;
    if (!ho_is_loop(h, F3, p)) return 0;
    const uint32_t L = p.len[h], n = L & HO_LEN;
    if (L & HO_OPEN) {
        if (kind) *kind = 1;
        return 0;
    }
    if (n < 3 || (max_edges && n > max_edges)) {
        if (kind) *kind = 2;
        return 0;
    }
    return n;
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_fcount(uint32_t F3, uint32_t max_edges, HoPtr p) {
    __shared__ uint32_t red[HO_NF][MC_WAVES];
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t kind = 0, n = 0;
    if (!p.hdr[0]) n = ho_fill_len(i, F3, max_edges, p, &kind);       // a flagged mesh counts nothing
    uint32_t tot[HO_NF];
    tot[0] = mc_block_total<1>(n > 3, red[0]);       // new vertices
    mc_block_excl(n == 3 ? 1u : n, red[1], tot[1]);  // new faces
    tot[2] = mc_block_total<1>(n > 0, red[2]);
    tot[3] = mc_block_total<1>(kind == 1, red[3]);
    tot[4] = mc_block_total<1>(kind == 2, red[4]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < HO_NF; ++q) p.sums[(uint64_t)blockIdx.x * HO_NF + q] = tot[q];
    }
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_ho_fscan(uint32_t nblk, HoPtr p, uint32_t *__restrict__ counts) {
    uint64_t tot[HO_NF];
    mc_scan_totals_n<HO_NF>(p.sums, nblk, tot);      // new faces <= boundary edges <= 3 F < 2^31
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < HO_NF; ++q) counts[q] = (uint32_t)tot[q];
        counts[HO_NF] = p.hdr[0];
    }
}

// the input is the prefix of the output
__global__ __launch_bounds__(MC_BLOCK) void k_ho_copy(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                      const int32_t *__restrict__ faces, uint32_t F, HoPtr p, float *__restrict__ verts_out,
                                                      float *__restrict__ normals_out, int32_t *__restrict__ faces_out, uint32_t max_verts,
                                                      uint32_t max_faces) {
    if (p.hdr[0]) return;                            // a flagged mesh: nothing is written
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < V) mesh_emit_vertex(verts, normals, i, i, verts_out, normals_out, nullptr, max_verts);
    if (i < F && i < max_faces) {
#pragma unroll
        for (int q = 0; q < 3; ++q) faces_out[3 * (uint64_t)i + q] = faces[3 * (uint64_t)i + q];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_ho_fan(const float *__restrict__ verts, const int32_t *__restrict__ fa, uint32_t V, uint32_t F,
                                                     uint32_t max_edges, HoPtr p, float *__restrict__ verts_out, float *__restrict__ normals_out,
                                                     int32_t *faces_out, uint32_t max_verts, uint32_t max_faces) {
    __shared__ uint32_t red_v[MC_WAVES], red_f[MC_WAVES];
    if (p.hdr[0]) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x, F3 = 3 * F;
    const uint32_t n = ho_fill_len(i, F3, max_edges, p, nullptr), nf = n == 3 ? 1u : n;
    uint32_t tot;
    const uint64_t cv = (uint64_t)V + p.sums[(uint64_t)blockIdx.x * HO_NF] + mc_block_prefix<1>(n > 3, red_v);
    const uint64_t f0 = (uint64_t)F + p.sums[(uint64_t)blockIdx.x * HO_NF + 1] + mc_block_excl(nf, red_f, tot);
    if (!n || f0 + nf > max_faces || (n > 3 && cv >= max_verts)) return;
    uint32_t h = i;
    if (n == 3) {                                    // a -> b -> c -> a: the face (b, a, c)
        const uint32_t h1 = p.nxt[h], h2 = h1 < F3 ? p.nxt[h1] : HO_NONE;
        if (h2 >= F3) return;                        // (a simple loop has every next)
        faces_out[3 * f0] = (int32_t)ho_from(fa, h1);
        faces_out[3 * f0 + 1] = (int32_t)ho_from(fa, h);
        faces_out[3 * f0 + 2] = (int32_t)ho_from(fa, h2);
        return;
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < n; ++j) {               // the fan in loop order; the centroid's sum in the same order
        const uint32_t a = ho_from(fa, h), b = ho_to(fa, h);
        const uint64_t d = 3 * (f0 + j);
        faces_out[d] = (int32_t)b;
        faces_out[d + 1] = (int32_t)a;
        faces_out[d + 2] = (int32_t)cv;
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += (double)verts[3 * (uint64_t)a + q];
        h = p.nxt[h];
        if (h >= F3) return;
    }
    float c[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        c[q] = (float)(s[q] / (double)n);
        verts_out[3 * cv + q] = c[q];
    }
    if (!normals_out) return;
    double m[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < n; ++j) {               // (p1 - p0) x (p2 - p0) of the faces this thread has just written
        const uint64_t d = 3 * (f0 + j);
        const uint64_t b = (uint64_t)faces_out[d], a = (uint64_t)faces_out[d + 1];
        double e1[3], e2[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double pb = (double)verts[3 * b + q];
            e1[q] = (double)verts[3 * a + q] - pb;
            e2[q] = (double)c[q] - pb;
        }
        m[0] += e1[1] * e2[2] - e1[2] * e2[1];
        m[1] += e1[2] * e2[0] - e1[0] * e2[2];
        m[2] += e1[0] * e2[1] - e1[1] * e2[0];
    }
    const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) normals_out[3 * cv + q] = l > 0.0 ? (float)(m[q] / l) : 0.0f;
}

int ho_check_dims(uint32_t V, uint32_t F) { return (V >= (1u << 31) || F > HO_MAX_F) ? CNERF_EINVAL : CNERF_OK; }

}  // namespace

extern "C" {

int cnerf_mesh_holes_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (const int rc = ho_check_dims(V, F)) return rc;
    if (!bytes_host) return CNERF_ENULL;
    HoPtr p;
    *bytes_host = ho_carve(nullptr, V, F, p);
    return CNERF_OK;
}

int cnerf_mesh_topology(const int32_t *faces, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream) {
    if (const int rc = ho_check_dims(V, F)) return rc;
    if (!F) return CNERF_OK;
    if (!faces || !ws || !counts) return CNERF_ENULL;
    HoPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, ho_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    ho_analyse(faces, V, F, 1, p, st);
    hipLaunchKernelGGL(k_ho_tcount, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, faces, V, F, p);
    hipLaunchKernelGGL(k_ho_tscan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, cn_div_up(p.n, MC_BLOCK), p, counts);
    return cn_launch_status();
}

int cnerf_mesh_topology_loops(uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, int32_t *loop_lengths, uint32_t max_loops, void *stream) {
    if (const int rc = ho_check_dims(V, F)) return rc;
    if (!F || !max_loops) return CNERF_OK;
    if (!ws || !loop_lengths) return CNERF_ENULL;
    HoPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, ho_carve(ws, V, F, p))) return rc;
    hipLaunchKernelGGL(k_ho_tloops, mesh_grid(p.n), dim3(MC_BLOCK), 0, CN_STREAM(stream), 3 * F, p, loop_lengths, max_loops);
    return cn_launch_status();
}

int cnerf_mesh_holes_count(const int32_t *faces, uint32_t V, uint32_t F, uint32_t max_edges, void *ws, uint64_t ws_bytes, uint32_t *counts,
                           void *stream) {
    if (const int rc = ho_check_dims(V, F)) return rc;
    if (max_edges == 1 || max_edges == 2) return CNERF_EINVAL;
    if (!F) return CNERF_OK;
    if (!faces || !ws || !counts) return CNERF_ENULL;
    HoPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, ho_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    ho_analyse(faces, V, F, 0, p, st);
    hipLaunchKernelGGL(k_ho_fcount, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, 3 * F, max_edges, p);
    hipLaunchKernelGGL(k_ho_fscan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, cn_div_up(p.n, MC_BLOCK), p, counts);
    return cn_launch_status();
}

int cnerf_mesh_holes_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t max_edges, void *ws,
                          uint64_t ws_bytes, float *verts_out, float *normals_out, int32_t *faces_out, uint32_t max_verts, uint32_t max_faces,
                          void *stream) {
    if (const int rc = ho_check_dims(V, F)) return rc;
    if (max_edges == 1 || max_edges == 2) return CNERF_EINVAL;
    if (!F) return CNERF_OK;
    if ((V && !verts) || !faces || !ws || (max_verts && !verts_out) || (max_faces && !faces_out)) return CNERF_ENULL;
    HoPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, ho_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    float *no = normals && max_verts ? normals_out : nullptr;
    hipLaunchKernelGGL(k_ho_copy, mesh_grid(V > F ? V : F), dim3(MC_BLOCK), 0, st, verts, normals, V, faces, F, p, verts_out, no, faces_out,
                       max_verts, max_faces);
    hipLaunchKernelGGL(k_ho_fan, mesh_grid(p.n), dim3(MC_BLOCK), 0, st, verts, faces, V, F, max_edges, p, verts_out, no, faces_out, max_verts,
                       max_faces);
    return cn_launch_status();
}

}  // extern "C"
