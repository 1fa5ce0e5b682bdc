// Quadric edge-collapse decimation on the device (cnerf_mesh_decimate_*; Garland & Heckbert 1997) to a target face count, in parallel rounds
// of independent collapses.  Same conventions as mesh_clean.hip: the caller's stream and workspace, no allocation, no host sync; counts[4] =
// (referenced vertices, live faces, collapses in this call, flags) is the one host read after init and after each round.  Every rule is
// fixed, so the output is bit-reproducible; only + - * / sqrt in fp64 under -ffp-contract=off, restated bit for bit by
// tests/qem_restatement.py.  The only atomics are integer ones whose result does not depend on their order (counts, atomicMin, list slots
// whose order nothing reads).
//
// Input: edge-manifold and consistently oriented (every undirected edge in at most two faces, which use it in opposite directions), no face
// repeating an index.  flags bit 0: an index outside [0, V); bit 1: a non-manifold or inconsistently oriented edge; bit 2: a repeated index.
//
// Rules
//   quadrics  : a face of nonzero area has area * (n n^T, n d, d^2) in fp64, n its unit normal, d = -n . p0, from the float32 positions.
//               A vertex sums its faces' quadrics in increasing face index, once at init; a collapse (u, v), u < v, gives Q_u + Q_v.
//   boundary  : a vertex on an edge with one face.  Boundary vertices never move and are never removed.  Candidates: edges with two faces and
//               at most one boundary endpoint.  With one, the edge collapses onto it and the cost is evaluated there; otherwise min(u, v) is
//               kept at x = m + A+ (-b - A m), m the midpoint (mesh_qef.h: Jacobi, eigenvalues < 1e-3 lambda_max dropped; x = m when A = 0).
//               Every collapse removes one vertex and two faces.
//   cost, key : cost = x^T A x + 2 b^T x + c, clamped at 0, rounded to float32; key = (cost bits) << 32 | edge id, the edge id 3 f + k of the
//               canonical half-edge (f[k], f[k+1]) (f[k] < f[k+1], or no twin) in this round's face order.
//   valid     : both endpoints in <= DC_MAX_DEG faces; the endpoints share exactly 2 neighbours (link condition); no two faces that survive
//               around the kept vertex have one vertex set (no tetrahedron collapse); no surviving face around u or v with n_old != 0 gets
//               n_new . n_old <= 0.2 |n_new| |n_old|, n = (p1 - p0) x (p2 - p0) in fp64 with the kept vertex at its float32 position.
//   select    : every valid edge takes the atomicMin of its key on both endpoints; a pre-winner holds both and takes the atomicMin of its key
//               on every vertex of every face around u or v; a winner holds all of those.  Winners have disjoint neighbourhoods, so their
//               collapses touch disjoint faces; the cheapest valid edge always wins.  When the winners would take F below the target, only
//               the ceil((F - target) / 2) smallest keys are applied (radix select on the device), so F' is target or target - 1.
//   apply     : the kept vertex gets (float) x and Q_u + Q_v; the removed one is remapped in the faces, the two faces of the edge are dropped,
//               the rest compacted by scan in order.
//   emit      : surviving input faces in input order, remapped; the referenced vertices in increasing input index, old_index, normals.
//
// Workspace (its first part does not depend on F, so a round can pass the live F): header | positions f32 [V][3] | quadrics f64 [V][10] |
//   degree u32 [V] | list end u32 [V] | boundary u8 [V] | remap u32 [V] | endpoint key u64 [V] | neighbourhood key u64 [V] | faces i32 [F][3]
//   -- per round: working faces i32 [F][3] | vertex -> face list u32 [3F] | twin u32 [3F] | edge key u64 [3F] | dropped u8 [F] |
//   workgroup totals uint2 [max(V, F) / 256] | pre-winners u32 [V/2 + 1] | winner keys u64 [V/2 + 1]
//
// A round (init: load, vsum, scan, offsets, fill, sort, twin with the manifold check, quadric):
//   k_dc_clear   : per vertex: degree, boundary, keys reset, remap = identity
//   k_dc_deg     : per face: working copy, degrees (atomicAdd)
//   k_dc_vsum / k_dc_scan / k_dc_offsets : exclusive scan of the degrees; k_dc_fill appends each face to its vertices' lists (atomicAdd on
//                  the list end, which ends at start + degree).  Order in a list matters only for the init sums, which sort it first.
//   k_dc_twin    : per half-edge its twin (the face using it backwards) and the boundary marks
//   k_dc_cand    : per canonical half-edge: validity, position, cost, key; atomicMin on both endpoints
//   k_dc_pre     : pre-winners: atomicMin on their neighbourhood, appended to a list
//   k_dc_win     : winners appended to a list of keys
//   k_dc_select  : one workgroup: the key limit (all, or the n-th smallest by an 8-bit radix select)
//   k_dc_apply   : the winners under the limit write position, quadric, remap and the two dropped faces
//   k_dc_fcount / k_dc_fscan / k_dc_compact : surviving faces, counts, compaction into the persistent faces
#include "common.h"
#include "mesh_common.h"
#include "mesh_qef.h"

#define DC_BAD_INDEX 1u
#define DC_NON_MANIFOLD 2u
#define DC_REPEATED 4u
#define DC_NONE 0xffffffffu
#define DC_NOKEY 0xffffffffffffffffull               // no key: the cost bits of a NaN, which a clamped cost never has
#define DC_MAX_DEG 32
#define DC_MAX_F 0x55555555u                         // 3 F - 1 edge ids fit the 32 low bits of a key
#define DC_FLIP 0.2

namespace {

enum { H_FLAGS = 0, H_REFS = 1, H_NPRE = 2, H_NWIN = 3, H_NAPPLY = 4, H64_LIM = 4 };     // uint32 slots of the header; H64_LIM: uint64 slot

struct DcPtr {
    uint32_t *hdr;
    float *pos;
    double *quad;
    uint32_t *deg, *end;
    uint8_t *bnd;
    uint32_t *remap;
    unsigned long long *vkey, *nkey;
    int32_t *faces, *work;
    uint32_t *list, *twin;
    uint64_t *ekey;
    uint8_t *dead;
    uint2 *sums;
    uint32_t *pre;
    uint64_t *win;
    uint32_t cap;
};

// the workspace: its regions in order -> total bytes (ws == nullptr: the size only).  The V-sized regions come first, so a round can pass
// the live F and find them where init put them.
uint64_t dc_carve(void *ws, uint64_t V, uint64_t F, DcPtr &p) {
    MeshCarve c(ws);
    p.cap = (uint32_t)(V / 2 + 1);                   // pre-winners hold both endpoints' minima: a matching, at most V / 2 edges
    p.hdr = c.header();
    p.pos = c.take<float>(3 * V);
    p.quad = c.take<double>(10 * V);
    p.deg = c.take<uint32_t>(V);
    p.end = c.take<uint32_t>(V);
    p.bnd = c.take<uint8_t>(V);
    p.remap = c.take<uint32_t>(V);
    p.vkey = c.take<unsigned long long>(V);
    p.nkey = c.take<unsigned long long>(V);
    p.faces = c.take<int32_t>(3 * F);
    p.work = c.take<int32_t>(3 * F);
    p.list = c.take<uint32_t>(3 * F);
    p.twin = c.take<uint32_t>(3 * F);
    p.ekey = c.take<uint64_t>(3 * F);
    p.dead = c.take<uint8_t>(F);
    const uint64_t n = V > F ? V : F;
    p.sums = c.take<uint2>(cn_div_up64(n ? n : 1, MC_BLOCK));
    p.pre = c.take<uint32_t>(p.cap);
    p.win = c.take<uint64_t>(p.cap);
    return c.total();
}

__device__ __forceinline__ uint32_t dc_next(uint32_t k) { return k == 2 ? 0 : k + 1; }

// ------------------------------------------------------------------------------------------------ vertex -> face lists
__global__ __launch_bounds__(MC_BLOCK) void k_dc_clear(uint32_t V, DcPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    p.deg[v] = 0;
    p.bnd[v] = 0;
    p.remap[v] = v;
    p.vkey[v] = DC_NOKEY;
    p.nkey[v] = DC_NOKEY;
}

// init: copy of the input faces, the flags, degrees of the faces whose indices are in range
__global__ __launch_bounds__(MC_BLOCK) void k_dc_load(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, DcPtr p) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    const bool ok = mesh_face(faces, f, V, t);
#pragma unroll
    for (int q = 0; q < 3; ++q) p.faces[3 * (uint64_t)f + q] = (int32_t)t[q];
    if (!ok) {
        atomicOr(p.hdr + H_FLAGS, DC_BAD_INDEX);
        return;
    }
    if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) atomicOr(p.hdr + H_FLAGS, DC_REPEATED);
#pragma unroll
    for (int q = 0; q < 3; ++q) atomicAdd(p.deg + t[q], 1u);
}

// round: working copy of the live faces, degrees, dropped marks and list counters reset
__global__ __launch_bounds__(MC_BLOCK) void k_dc_deg(uint32_t F, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f == 0) p.hdr[H_NPRE] = p.hdr[H_NWIN] = 0;
    if (f >= F) return;
    p.dead[f] = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int32_t t = p.faces[3 * (uint64_t)f + q];
        p.work[3 * (uint64_t)f + q] = t;
        atomicAdd(p.deg + t, 1u);
    }
}

// workgroup totals of (degree, referenced)
__global__ __launch_bounds__(MC_BLOCK) void k_dc_vsum(uint32_t V, DcPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t d = v < V ? p.deg[v] : 0;
    mesh_csr_totals(d, d ? 1u : 0u, p.sums);
}

// one workgroup: the shared scan of the workgroup totals.  refs != 0: the referenced vertices are the header's count (init)
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_dc_scan(uint32_t nblk, int refs, DcPtr p) {
    uint64_t cx, cy;
    mc_scan_totals(p.sums, nblk, cx, cy);            // sum of degrees = 3 F <= 2^32 - 1
    if (refs && threadIdx.x == 0) p.hdr[H_REFS] = (uint32_t)cy;
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_offsets(uint32_t V, DcPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t start = mesh_csr_start(p.sums[blockIdx.x].x, v < V ? p.deg[v] : 0, red);
    if (v < V) p.end[v] = start;                     // k_dc_fill advances it to start + degree
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_fill(const int32_t *__restrict__ fa, uint32_t F, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) p.list[atomicAdd(p.end + mesh_fv(fa, f, q), 1u)] = f;
}

// init: each vertex sorts its own list (increasing face index: the order of the quadric sums)
__global__ __launch_bounds__(MC_BLOCK) void k_dc_sort(uint32_t V, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    mesh_isort(p.list + (p.end[v] - p.deg[v]), p.deg[v]);
}

// per half-edge (a, b) of face f: its twin, the half-edge (b, a) of another face; no twin marks a and b as boundary.  check (init, no face
// repeating an index): flags bit 1 when (a, b) is used by another face too or (b, a) by more than one
__global__ __launch_bounds__(MC_BLOCK) void k_dc_twin(const int32_t *__restrict__ fa, uint32_t F, int check, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t he = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (he >= 3 * F) return;
    const uint32_t f = he / 3, k = he - 3 * f;
    const uint32_t a = mesh_fv(fa, f, k), b = mesh_fv(fa, f, dc_next(k));
    uint32_t tw = DC_NONE, ntw = 0;
    for (uint32_t i = p.end[b] - p.deg[b]; i < p.end[b]; ++i) {
        const uint32_t g = p.list[i];
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j)
            if (mesh_fv(fa, g, j) == b && mesh_fv(fa, g, dc_next(j)) == a) {
                tw = 3 * g + j;
                ++ntw;
            }
    }
    p.twin[he] = tw;
    if (tw == DC_NONE) {
        p.bnd[a] = 1;
        p.bnd[b] = 1;
    }
    if (check && !(p.hdr[H_FLAGS] & DC_REPEATED)) {          // (a repeated index is reported as such)
        uint32_t same = 0;
        for (uint32_t i = p.end[a] - p.deg[a]; i < p.end[a]; ++i) {
            const uint32_t g = p.list[i];
#pragma unroll
            for (uint32_t j = 0; j < 3; ++j) same += mesh_fv(fa, g, j) == a && mesh_fv(fa, g, dc_next(j)) == b;
        }
        if (same != 1 || ntw > 1) atomicOr(p.hdr + H_FLAGS, DC_NON_MANIFOLD);
    }
}

// plane quadric of face g: area (n n^T, n d, d^2), 10 doubles (A00 A01 A02 A11 A12 A22 b0 b1 b2 c); false for zero area or non-finite
__device__ __forceinline__ bool dc_face_quadric(const float *__restrict__ P, const int32_t *__restrict__ fa, uint32_t g, double q[10]) {
    double p[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[i][a] = (double)P[3 * (uint64_t)mesh_fv(fa, g, i) + a];
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[1][a] - p[0][a];
        e2[a] = p[2][a] - p[0][a];
    }
    const double m[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double mm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    if (!(mm > 0.0) || !(mm < 1e300)) return false;
    const double n[3] = {m[0] / mm, m[1] / mm, m[2] / mm}, area = 0.5 * mm;
    double d = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) d -= n[a] * p[0][a];
    q[0] = area * n[0] * n[0];
    q[1] = area * n[0] * n[1];
    q[2] = area * n[0] * n[2];
    q[3] = area * n[1] * n[1];
    q[4] = area * n[1] * n[2];
    q[5] = area * n[2] * n[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[6 + a] = area * n[a] * d;
    q[9] = area * d * d;
    return true;
}

// init: positions copied, quadrics summed over each vertex's faces in increasing face index
__global__ __launch_bounds__(MC_BLOCK) void k_dc_quadric(const float *__restrict__ verts, uint32_t V, DcPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) p.pos[3 * (uint64_t)v + a] = verts[3 * (uint64_t)v + a];
    double Q[10];
#pragma unroll
    for (int j = 0; j < 10; ++j) Q[j] = 0.0;
    if (!(p.hdr[H_FLAGS] & DC_BAD_INDEX)) {
        for (uint32_t i = p.end[v] - p.deg[v]; i < p.end[v]; ++i) {
            double q[10];
            if (!dc_face_quadric(verts, p.faces, p.list[i], q)) continue;
#pragma unroll
            for (int j = 0; j < 10; ++j) Q[j] += q[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) p.quad[10 * (uint64_t)v + j] = Q[j];
}

__global__ void k_dc_report(uint32_t F, DcPtr p, uint32_t *__restrict__ counts) {
    counts[0] = p.hdr[H_REFS];
    counts[1] = F;
    counts[2] = 0;
    counts[3] = p.hdr[H_FLAGS];
}

// ------------------------------------------------------------------------------------------------ candidates
// e-th neighbour entry of vertex c: the other two vertices of each of its faces, in face order from c
__device__ __forceinline__ uint32_t dc_nbr(const int32_t *__restrict__ fa, const DcPtr &p, uint32_t c, uint32_t e) {
    const uint32_t g = p.list[p.end[c] - p.deg[c] + (e >> 1)];
    uint32_t j = 0;
    while (j < 2 && mesh_fv(fa, g, j) != c) ++j;
    return mesh_fv(fa, g, (j + 1 + (e & 1)) % 3);
}

// link condition: u and v share exactly two neighbours
__device__ bool dc_link(const int32_t *__restrict__ fa, const DcPtr &p, uint32_t u, uint32_t v) {
    const uint32_t nu = 2 * p.deg[u], nv = 2 * p.deg[v];
    uint32_t common = 0;
    for (uint32_t e = 0; e < nv; ++e) {
        const uint32_t w = dc_nbr(fa, p, v, e);
        if (w == u) continue;
        bool seen = false;
        for (uint32_t e2 = 0; e2 < e && !seen; ++e2) seen = dc_nbr(fa, p, v, e2) == w;
        if (seen) continue;
        bool in_u = false;
        for (uint32_t e3 = 0; e3 < nu && !in_u; ++e3) in_u = dc_nbr(fa, p, u, e3) == w;
        if (in_u && ++common > 2) return false;
    }
    return common == 2;
}

// i-th face around u then v (i < deg u + deg v)
__device__ __forceinline__ uint32_t dc_around(const DcPtr &p, uint32_t u, uint32_t v, uint32_t i, uint32_t &c) {
    const uint32_t du = p.deg[u];
    c = i < du ? u : v;
    return p.list[p.end[c] - p.deg[c] + (i < du ? i : i - du)];
}

// no two faces that survive around the kept vertex share their vertex set: each holds the kept vertex, so compare the other two
__device__ bool dc_distinct(const int32_t *__restrict__ fa, const DcPtr &p, uint32_t u, uint32_t v, uint32_t f, uint32_t g) {
    const uint32_t n = p.deg[u] + p.deg[v];
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c;
        const uint32_t h = dc_around(p, u, v, i, c);
        if (h == f || h == g) continue;
        uint32_t j = 0;
        while (j < 2 && mesh_fv(fa, h, j) != c) ++j;
        uint32_t x0 = mesh_fv(fa, h, (j + 1) % 3), x1 = mesh_fv(fa, h, (j + 2) % 3);
        if (x0 > x1) { const uint32_t t = x0; x0 = x1; x1 = t; }
        for (uint32_t i2 = 0; i2 < i; ++i2) {
            uint32_t c2;
            const uint32_t h2 = dc_around(p, u, v, i2, c2);
            if (h2 == f || h2 == g) continue;
            uint32_t j2 = 0;
            while (j2 < 2 && mesh_fv(fa, h2, j2) != c2) ++j2;
            uint32_t y0 = mesh_fv(fa, h2, (j2 + 1) % 3), y1 = mesh_fv(fa, h2, (j2 + 2) % 3);
            if (y0 > y1) { const uint32_t t = y0; y0 = y1; y1 = t; }
            if (x0 == y0 && x1 == y1) return false;
        }
    }
    return true;
}

struct DcPlace {
    uint32_t kept, removed;
    double Q[10];
    float P[3];                                      // the kept vertex's new position: (float) x
    float cost;
};

// position and cost of collapsing (u, v), u < v
__device__ void dc_place(const DcPtr &p, uint32_t u, uint32_t v, DcPlace &r) {
    const bool bu = p.bnd[u], bv = p.bnd[v];
#pragma unroll
    for (int j = 0; j < 10; ++j) r.Q[j] = p.quad[10 * (uint64_t)u + j] + p.quad[10 * (uint64_t)v + j];
    double x[3];
    if (bu || bv) {
        r.kept = bu ? u : v;
        r.removed = bu ? v : u;
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = (double)p.pos[3 * (uint64_t)r.kept + a];
    } else {
        r.kept = u;
        r.removed = v;
        double m[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = ((double)p.pos[3 * (uint64_t)u + a] + (double)p.pos[3 * (uint64_t)v + a]) * 0.5;
        qef_solve(r.Q, r.Q + 6, m, x);
    }
    const double *s = r.Q;
    const double ax[3] = {s[0] * x[0] + s[1] * x[1] + s[2] * x[2], s[1] * x[0] + s[3] * x[1] + s[4] * x[2], s[2] * x[0] + s[4] * x[1] + s[5] * x[2]};
    const double xax = x[0] * ax[0] + x[1] * ax[1] + x[2] * ax[2];
    const double bx = s[6] * x[0] + s[7] * x[1] + s[8] * x[2];
    const double cost = xax + 2.0 * bx + s[9];
    r.cost = (float)(cost > 0.0 ? cost : 0.0);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.P[a] = (float)x[a];
}

__device__ __forceinline__ void dc_cross(const double p[3][3], double n[3]) {
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p[1][a] - p[0][a];
        e2[a] = p[2][a] - p[0][a];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// no surviving face around u or v turns by 78.5 degrees or more (or to zero area) with u and v at P
__device__ bool dc_no_flip(const int32_t *__restrict__ fa, const DcPtr &p, uint32_t u, uint32_t v, uint32_t f, uint32_t g, const float P[3]) {
    const uint32_t n = p.deg[u] + p.deg[v];
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c;
        const uint32_t h = dc_around(p, u, v, i, c);
        if (h == f || h == g) continue;
        double po[3][3], pn[3][3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const uint32_t t = mesh_fv(fa, h, q);
            const bool moved = t == u || t == v;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                po[q][a] = (double)p.pos[3 * (uint64_t)t + a];
                pn[q][a] = moved ? (double)P[a] : po[q][a];
            }
        }
        double no[3], nw[3];
        dc_cross(po, no);
        const double nno = no[0] * no[0] + no[1] * no[1] + no[2] * no[2];
        if (!(nno > 0.0)) continue;
        dc_cross(pn, nw);
        const double nnw = nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2];
        const double dot = nw[0] * no[0] + nw[1] * no[1] + nw[2] * no[2];
        if (dot <= DC_FLIP * sqrt(nnw) * sqrt(nno)) return false;
    }
    return true;
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_cand(uint32_t F, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t he = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (he >= 3 * F) return;
    const int32_t *fa = p.work;
    const uint32_t f = he / 3, k = he - 3 * f;
    const uint32_t u = mesh_fv(fa, f, k), v = mesh_fv(fa, f, dc_next(k)), tw = p.twin[he];
    uint64_t key = DC_NOKEY;
    if (tw != DC_NONE && u < v && !(p.bnd[u] && p.bnd[v]) && p.deg[u] <= DC_MAX_DEG && p.deg[v] <= DC_MAX_DEG && dc_link(fa, p, u, v) &&
        dc_distinct(fa, p, u, v, f, tw / 3)) {
        DcPlace r;
        dc_place(p, u, v, r);
        if (dc_no_flip(fa, p, u, v, f, tw / 3, r.P)) key = ((uint64_t)__float_as_uint(r.cost) << 32) | he;
    }
    p.ekey[he] = key;
    if (key != DC_NOKEY) {
        atomicMin(p.vkey + u, (unsigned long long)key);
        atomicMin(p.vkey + v, (unsigned long long)key);
    }
}

// ------------------------------------------------------------------------------------------------ independent selection
__global__ __launch_bounds__(MC_BLOCK) void k_dc_pre(uint32_t F, DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t he = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (he >= 3 * F) return;
    const uint64_t key = p.ekey[he];
    if (key == DC_NOKEY) return;
    const int32_t *fa = p.work;
    const uint32_t f = he / 3, k = he - 3 * f;
    const uint32_t u = mesh_fv(fa, f, k), v = mesh_fv(fa, f, dc_next(k));
    if (p.vkey[u] != key || p.vkey[v] != key) return;
    const uint32_t n = p.deg[u] + p.deg[v];
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t c;
        const uint32_t h = dc_around(p, u, v, i, c);
#pragma unroll
        for (int q = 0; q < 3; ++q) atomicMin(p.nkey + mesh_fv(fa, h, q), (unsigned long long)key);
    }
    const uint32_t slot = atomicAdd(p.hdr + H_NPRE, 1u);
    if (slot < p.cap) p.pre[slot] = he;
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_win(DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= p.hdr[H_NPRE] || i >= p.cap) return;
    const int32_t *fa = p.work;
    const uint32_t he = p.pre[i];
    const uint64_t key = p.ekey[he];
    const uint32_t f = he / 3, k = he - 3 * f;
    const uint32_t u = mesh_fv(fa, f, k), v = mesh_fv(fa, f, dc_next(k));
    const uint32_t n = p.deg[u] + p.deg[v];
    for (uint32_t j = 0; j < n; ++j) {
        uint32_t c;
        const uint32_t h = dc_around(p, u, v, j, c);
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (p.nkey[mesh_fv(fa, h, q)] != key) return;
    }
    const uint32_t slot = atomicAdd(p.hdr + H_NWIN, 1u);
    if (slot < p.cap) p.win[slot] = key;
}

// one workgroup: how many winners apply and the key limit.  All of them unless they take F below the target; then the n = ceil((F - target)
// / 2) smallest keys: the n-th smallest found by an 8-bit radix select over the (distinct) winner keys.
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_dc_select(uint32_t F, uint32_t target, DcPtr p) {
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_rank;
    const uint32_t nw = p.hdr[H_NWIN] < p.cap ? p.hdr[H_NWIN] : p.cap;
    uint32_t n = nw;
    if ((uint64_t)F < (uint64_t)target + 2ull * nw) n = F > target ? (F - target + 1) / 2 : 0;
    uint64_t lim = DC_NOKEY;                         // every key is below it
    if (n == 0) {
        lim = 0;
    } else if (n < nw) {
        uint64_t prefix = 0, mask = 0;
        uint32_t rank = n;
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (uint32_t d = threadIdx.x; d < 256; d += MC_SCAN_BLOCK) hist[d] = 0;
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < nw; i += MC_SCAN_BLOCK) {
                const uint64_t key = p.win[i];
                if ((key & mask) == prefix) atomicAdd(hist + ((key >> shift) & 255), 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t cum = 0, d = 0;
                for (; d < 255 && cum + hist[d] < rank; ++d) cum += hist[d];
                s_prefix = prefix | ((uint64_t)d << shift);
                s_rank = rank - cum;
            }
            __syncthreads();
            prefix = s_prefix;
            rank = s_rank;
            mask |= 255ull << shift;
        }
        lim = prefix + 1;                            // the n-th smallest key is `prefix`
    }
    if (threadIdx.x == 0) {
        p.hdr[H_NAPPLY] = n;
        ((uint64_t *)p.hdr)[H64_LIM] = lim;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_apply(DcPtr p) {
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= p.hdr[H_NWIN] || i >= p.cap) return;
    const uint64_t key = p.win[i];
    if (key >= ((const uint64_t *)p.hdr)[H64_LIM]) return;
    const int32_t *fa = p.work;
    const uint32_t he = (uint32_t)key, f = he / 3, k = he - 3 * f;
    const uint32_t u = mesh_fv(fa, f, k), v = mesh_fv(fa, f, dc_next(k));
    DcPlace r;
    dc_place(p, u, v, r);                            // as k_dc_cand computed it: the neighbourhood is the winner's alone
#pragma unroll
    for (int a = 0; a < 3; ++a) p.pos[3 * (uint64_t)r.kept + a] = r.P[a];
#pragma unroll
    for (int j = 0; j < 10; ++j) p.quad[10 * (uint64_t)r.kept + j] = r.Q[j];
    p.remap[r.removed] = r.kept;
    p.dead[f] = 1;
    p.dead[p.twin[he] / 3] = 1;
}

// ------------------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(MC_BLOCK) void k_dc_fcount(uint32_t F, DcPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t t = mc_block_total<1>(f < F && !p.dead[f], red);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = make_uint2(t, 0);
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_dc_fscan(uint32_t F, uint32_t nblk, DcPtr p, uint32_t *__restrict__ counts) {
    const uint32_t flags = p.hdr[H_FLAGS];
    if (flags & DC_BAD_INDEX) {
        if (threadIdx.x == 0) {
            counts[0] = p.hdr[H_REFS];
            counts[1] = F;
            counts[2] = 0;
            counts[3] = flags;
        }
        return;
    }
    uint64_t cf, c0;
    mc_scan_totals(p.sums, nblk, cf, c0);
    if (threadIdx.x == 0) {
        const uint32_t n = p.hdr[H_NAPPLY], refs = p.hdr[H_REFS] - n;     // a collapse unreferences exactly its removed vertex
        p.hdr[H_REFS] = refs;
        counts[0] = refs;
        counts[1] = (uint32_t)cf;
        counts[2] = n;
        counts[3] = flags;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_compact(uint32_t F, DcPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    if (p.hdr[H_FLAGS] & DC_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t keep = f < F && !p.dead[f];
    const uint32_t k = p.sums[blockIdx.x].x + mc_block_prefix<1>(keep, red);
    if (!keep) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) p.faces[3 * (uint64_t)k + q] = (int32_t)p.remap[p.work[3 * (uint64_t)f + q]];
}

// ------------------------------------------------------------------------------------------------ emit
__global__ __launch_bounds__(MC_BLOCK) void k_dc_emark(uint32_t F, DcPtr p) {
    if (p.hdr[H_FLAGS]) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) p.deg[p.faces[3 * (uint64_t)f + q]] = 1;
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_ecount(uint32_t V, DcPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t t = mc_block_total<1>(v < V && p.deg[v], red);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = make_uint2(t, 0);
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_everts(uint32_t V, DcPtr p, const float *__restrict__ normals, float *__restrict__ verts_out,
                                                        float *__restrict__ normals_out, int32_t *__restrict__ old_index, uint32_t max_verts) {
    __shared__ uint32_t red[MC_WAVES];
    if (p.hdr[H_FLAGS]) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t ref = v < V && p.deg[v];
    const uint32_t k = p.sums[blockIdx.x].x + mc_block_prefix<1>(ref, red);
    if (!ref) return;
    p.end[v] = k;                                    // new index
    mesh_emit_vertex(p.pos, normals, v, k, verts_out, normals_out, old_index, max_verts);
}

__global__ __launch_bounds__(MC_BLOCK) void k_dc_efaces(uint32_t F, DcPtr p, int32_t *__restrict__ faces_out, uint32_t max_faces) {
    if (p.hdr[H_FLAGS]) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F || f >= max_faces) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) faces_out[3 * (uint64_t)f + q] = (int32_t)p.end[p.faces[3 * (uint64_t)f + q]];
}

int dc_check_dims(uint32_t V, uint32_t F) { return (V >= (1u << 31) || F >= (1u << 31) || F > DC_MAX_F) ? CNERF_EINVAL : CNERF_OK; }

// vertex -> face lists of the faces `fa` (F of them): degrees already counted; init sorts the lists and checks the edges
void dc_lists(const int32_t *fa, uint32_t V, uint32_t F, int init, const DcPtr &p, hipStream_t st) {
    hipLaunchKernelGGL(k_dc_vsum, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_dc_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (uint32_t)cn_div_up64(V, MC_BLOCK), init, p);
    hipLaunchKernelGGL(k_dc_offsets, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_dc_fill, mesh_grid(F), dim3(MC_BLOCK), 0, st, fa, F, p);
    if (init) hipLaunchKernelGGL(k_dc_sort, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_dc_twin, mesh_grid(3ull * F), dim3(MC_BLOCK), 0, st, fa, F, init, p);
}

}  // namespace

extern "C" {

int cnerf_mesh_decimate_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (const int rc = dc_check_dims(V, F)) return rc;
    if (!bytes_host) return CNERF_ENULL;
    DcPtr p;
    *bytes_host = dc_carve(nullptr, V, F, p);
    return CNERF_OK;
}

int cnerf_mesh_decimate_init(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts,
                             void *stream) {
    if (const int rc = dc_check_dims(V, F)) return rc;
    if ((V && !verts) || (F && !faces) || !ws || !counts) return CNERF_ENULL;
    DcPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, dc_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(ws, 0, 256, st)) return rc;
    if (V) hipLaunchKernelGGL(k_dc_clear, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    if (F) hipLaunchKernelGGL(k_dc_load, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, p);
    if (V) {
        if (F) dc_lists(p.faces, V, F, 1, p, st);
        else hipLaunchKernelGGL(k_dc_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, 0u, 1, p);    // (no degrees: no referenced vertex)
        hipLaunchKernelGGL(k_dc_quadric, mesh_grid(V), dim3(MC_BLOCK), 0, st, verts, V, p);
    }
    hipLaunchKernelGGL(k_dc_report, dim3(1), dim3(1), 0, st, F, p, counts);
    return cn_launch_status();
}

int cnerf_mesh_decimate_round(uint32_t V, uint32_t F, uint32_t target_faces, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream) {
    if (const int rc = dc_check_dims(V, F)) return rc;
    if (!ws || !counts) return CNERF_ENULL;
    DcPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, dc_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    if (!F || !V) {
        hipLaunchKernelGGL(k_dc_report, dim3(1), dim3(1), 0, st, F, p, counts);
        return cn_launch_status();
    }
    hipLaunchKernelGGL(k_dc_clear, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_dc_deg, mesh_grid(F), dim3(MC_BLOCK), 0, st, F, p);
    dc_lists(p.work, V, F, 0, p, st);
    hipLaunchKernelGGL(k_dc_cand, mesh_grid(3ull * F), dim3(MC_BLOCK), 0, st, F, p);
    hipLaunchKernelGGL(k_dc_pre, mesh_grid(3ull * F), dim3(MC_BLOCK), 0, st, F, p);
    hipLaunchKernelGGL(k_dc_win, mesh_grid(p.cap), dim3(MC_BLOCK), 0, st, p);
    hipLaunchKernelGGL(k_dc_select, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, F, target_faces, p);
    hipLaunchKernelGGL(k_dc_apply, mesh_grid(p.cap), dim3(MC_BLOCK), 0, st, p);
    hipLaunchKernelGGL(k_dc_fcount, mesh_grid(F), dim3(MC_BLOCK), 0, st, F, p);
    hipLaunchKernelGGL(k_dc_fscan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, F, (uint32_t)cn_div_up64(F, MC_BLOCK), p, counts);
    hipLaunchKernelGGL(k_dc_compact, mesh_grid(F), dim3(MC_BLOCK), 0, st, F, p);
    return cn_launch_status();
}

int cnerf_mesh_decimate_emit(const float *normals, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out,
                             int32_t *faces_out, int32_t *old_index, uint32_t max_verts, uint32_t max_faces, void *stream) {
    if (const int rc = dc_check_dims(V, F)) return rc;
    if (!ws || (max_verts && !verts_out) || (max_faces && !faces_out)) return CNERF_ENULL;
    DcPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, dc_carve(ws, V, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    if (!V) return CNERF_OK;
    hipLaunchKernelGGL(k_dc_clear, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    if (F) hipLaunchKernelGGL(k_dc_emark, mesh_grid(F), dim3(MC_BLOCK), 0, st, F, p);
    hipLaunchKernelGGL(k_dc_ecount, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    hipLaunchKernelGGL(k_dc_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (uint32_t)cn_div_up64(V, MC_BLOCK), 0, p);
    hipLaunchKernelGGL(k_dc_everts, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p, normals, max_verts ? verts_out : nullptr,
                       max_verts ? normals_out : nullptr, max_verts ? old_index : nullptr, max_verts);
    if (F) hipLaunchKernelGGL(k_dc_efaces, mesh_grid(F), dim3(MC_BLOCK), 0, st, F, p, faces_out, max_faces);
    return cn_launch_status();
}

}  // extern "C"
