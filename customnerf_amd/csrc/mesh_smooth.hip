// Taubin lambda|mu smoothing (Taubin 1995) with uniform weights and area-weighted vertex normals on the device (cnerf_mesh_smooth_*), for any
// triangle mesh: clustering output need not be manifold.  Same conventions as mesh_clean.hip / mesh_decimate.hip: the caller's stream and
// workspace, no allocation, no host sync; flags (one device uint32 written by init) is the one host read per call.  The only atomics are
// integer ones whose result does not depend on their order (degrees, list slots, the flag bit): every list is sorted before anything reads
// it, so the output is bit-reproducible and tests/smooth_restatement.py restates it bit for bit.
//
// Input: verts float32 [V][3], faces int32 [F][3], optional normals float32 [V][3].  flags bit 0: an index outside [0, V); steps and
// normals then write nothing.  F > 0x2AAAAAAA is rejected (CNERF_EINVAL) so that the 6 F neighbour records fit a u32.
//
// Rules
//   neighbours : the distinct vertices that share an edge with v, in increasing index.  A face adds its distinct undirected edges only (a face
//                repeating an index adds one edge or none).  The records (one per edge end and face) are appended in arbitrary order, then
//                each vertex sorts its own and keeps the first of each run.
//   boundary   : a vertex one of whose edges lies in exactly one face (a run of length 1).  With pin_boundary it keeps its position bit for
//                bit; a vertex with no neighbours never moves.
//   step (s)   : Jacobi, every vertex reads the previous buffer.  sum = the neighbours' positions added in float32 in list order, starting
//                from the first; m = sum / (float) n; x' = x + s * (m - x), three rounded operations (-ffp-contract=off).  One iteration
//                is a lambda step, then a mu step when mu != 0.
//   normals    : face normal c = (p1 - p0) x (p2 - p0) = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x) in float32, e1 = p1 - p0,
//                e2 = p2 - p0.  A vertex adds the normals of its faces (a face counts once) in increasing face index to (0, 0, 0) in float32;
//                q = ax ax + ay ay + az az (left to right); with 0 < q < inf the normal is a / sqrt(q) (three divisions), otherwise the
//                input normal, or (0, 0, 0) without one.
//
// Workspace: header | per vertex: list start and count | boundary (uint2) [V] | record degree u32 [V] | record end u32 [V] | face degree
//   u32 [V] | face end u32 [V] | workgroup totals uint2 [V / 256] | neighbour records u32 [6F] | vertex -> face lists u32 [3F] | two position
//   buffers float32 [V][3].
//
// init (faces only):
//   k_sm_clear   : per vertex: degrees reset
//   k_sm_deg     : per face: index check (flags bit 0), degrees (atomicAdd): two records per distinct edge, one list slot per distinct vertex
//   k_sm_vsum / k_sm_scan / k_sm_offsets : exclusive scan of both degrees (mesh_common.h)
//   k_sm_fill    : per face: the records and the face list entries (atomicAdd on the list ends, which end at start + degree)
//   k_sm_sort    : per vertex: both lists sorted; neighbour runs collapsed to their first entry, boundary mark; flags out
// steps: k_sm_step per step, ping-pong between the two buffers, the last one into verts_out (k_sm_copy for zero iterations)
// normals: k_sm_normals per vertex, its faces' normals recomputed from `verts`
#include "common.h"
#include "mesh_common.h"

#define SM_BAD_INDEX 1u
#define SM_MAX_F 0x2AAAAAAAu                         // 6 F records fit a u32
#define SM_BOUNDARY 0x80000000u                      // in the count word of a vertex

namespace {

enum { H_FLAGS = 0 };                                // uint32 slots of the header

struct SmPtr {
    uint32_t *hdr;
    uint2 *nbr;                                      // (list start, distinct count | SM_BOUNDARY)
    uint32_t *deg, *end, *fdeg, *fend;
    uint2 *sums;
    uint32_t *rec, *flist;
    float *pos[2];
};

// the workspace: its regions in order -> total bytes (ws == nullptr: the size only)
uint64_t sm_carve(void *ws, uint64_t V, uint64_t F, SmPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.nbr = c.take<uint2>(V);
    p.deg = c.take<uint32_t>(V);
    p.end = c.take<uint32_t>(V);
    p.fdeg = c.take<uint32_t>(V);
    p.fend = c.take<uint32_t>(V);
    p.sums = c.take<uint2>(cn_div_up64(V ? V : 1, MC_BLOCK));
    p.rec = c.take<uint32_t>(6 * F);
    p.flist = c.take<uint32_t>(3 * F);
    p.pos[0] = c.take<float>(3 * V);
    p.pos[1] = c.take<float>(3 * V);
    return c.total();
}

// calls vert(u) for each distinct vertex u of face t and edge(a, b) for each of its distinct undirected edges: all three with three
// distinct vertices, the one between them with two, none with one
template <class Vert, class Edge>
__device__ __forceinline__ void sm_face(const uint32_t t[3], Vert vert, Edge edge) {
    const bool d01 = t[0] != t[1], d12 = t[1] != t[2], d02 = t[0] != t[2];
    vert(t[0]);
    if (d01 && d12 && d02) {
        vert(t[1]);
        vert(t[2]);
        edge(t[0], t[1]);
        edge(t[1], t[2]);
        edge(t[2], t[0]);
    } else if (d01 || d12) {
        const uint32_t o = d01 ? t[1] : t[2];
        vert(o);
        edge(t[0], o);
    }
}

// ------------------------------------------------------------------------------------------------ init: lists and boundary marks
__global__ __launch_bounds__(MC_BLOCK) void k_sm_clear(uint32_t V, SmPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    p.deg[v] = 0;
    p.fdeg[v] = 0;
}

__global__ __launch_bounds__(MC_BLOCK) void k_sm_deg(const int32_t *__restrict__ fa, uint32_t V, uint32_t F, SmPtr p) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    if (!mesh_face(fa, f, V, t)) {
        atomicOr(p.hdr + H_FLAGS, SM_BAD_INDEX);
        return;
    }
    sm_face(t, [&](uint32_t u) { atomicAdd(p.fdeg + u, 1u); }, [&](uint32_t a, uint32_t b) {
        atomicAdd(p.deg + a, 1u);
        atomicAdd(p.deg + b, 1u);
    });
}

// workgroup totals of (record degree, face degree)
__global__ __launch_bounds__(MC_BLOCK) void k_sm_vsum(uint32_t V, SmPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    mesh_csr_totals(v < V ? p.deg[v] : 0, v < V ? p.fdeg[v] : 0, p.sums);
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_sm_scan(uint32_t nblk, SmPtr p) {
    uint64_t cd, cf;
    mc_scan_totals(p.sums, nblk, cd, cf);            // 6 F and 3 F < 2^32
}

__global__ __launch_bounds__(MC_BLOCK) void k_sm_offsets(uint32_t V, SmPtr p) {
    __shared__ uint32_t red_d[MC_WAVES], red_f[MC_WAVES];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t sd = mesh_csr_start(p.sums[blockIdx.x].x, v < V ? p.deg[v] : 0, red_d);
    const uint32_t sf = mesh_csr_start(p.sums[blockIdx.x].y, v < V ? p.fdeg[v] : 0, red_f);
    if (v >= V) return;
    p.end[v] = sd;                                   // k_sm_fill advances both to start + degree
    p.fend[v] = sf;
}

__global__ __launch_bounds__(MC_BLOCK) void k_sm_fill(const int32_t *__restrict__ fa, uint32_t F, SmPtr p) {
    if (p.hdr[H_FLAGS] & SM_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = mesh_fv(fa, f, q);
    sm_face(t, [&](uint32_t u) { p.flist[atomicAdd(p.fend + u, 1u)] = f; }, [&](uint32_t a, uint32_t b) {
        p.rec[atomicAdd(p.end + a, 1u)] = b;
        p.rec[atomicAdd(p.end + b, 1u)] = a;
    });
}

// each vertex sorts its records and its faces; a run of equal records is one neighbour (its length: the faces on that edge)
__global__ __launch_bounds__(MC_BLOCK) void k_sm_sort(uint32_t V, SmPtr p, uint32_t *__restrict__ flags) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v == 0) flags[0] = p.hdr[H_FLAGS];
    if (v >= V || (p.hdr[H_FLAGS] & SM_BAD_INDEX)) return;
    const uint32_t d = p.deg[v], start = p.end[v] - d;
    uint32_t *l = p.rec + start;
    mesh_isort(l, d);
    uint32_t n = 0, bnd = 0;
    for (uint32_t i = 0; i < d;) {
        const uint32_t w = l[i];
        uint32_t j = i + 1;
        while (j < d && l[j] == w) ++j;
        bnd |= j - i == 1;
        l[n++] = w;                                  // n <= i: the run's first entry moves to the front
        i = j;
    }
    p.nbr[v] = make_uint2(start, n | (bnd ? SM_BOUNDARY : 0u));
    mesh_isort(p.flist + (p.fend[v] - p.fdeg[v]), p.fdeg[v]);
}

// ------------------------------------------------------------------------------------------------ steps
__global__ __launch_bounds__(MC_BLOCK) void k_sm_step(const float *__restrict__ src, float *__restrict__ dst, uint32_t V, float s, int pin,
                                                      SmPtr p) {
    if (p.hdr[H_FLAGS] & SM_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const uint64_t o = 3 * (uint64_t)v;
    float x0 = src[o], x1 = src[o + 1], x2 = src[o + 2];
    const uint2 nb = p.nbr[v];
    const uint32_t n = nb.y & ~SM_BOUNDARY;
    if (n && !(pin && (nb.y & SM_BOUNDARY))) {
        const uint32_t *l = p.rec + nb.x;
        uint64_t w = 3 * (uint64_t)l[0];
        float s0 = src[w], s1 = src[w + 1], s2 = src[w + 2];
        for (uint32_t i = 1; i < n; ++i) {
            w = 3 * (uint64_t)l[i];
            s0 += src[w];
            s1 += src[w + 1];
            s2 += src[w + 2];
        }
        const float c = (float)n;
        x0 = x0 + s * (s0 / c - x0);
        x1 = x1 + s * (s1 / c - x1);
        x2 = x2 + s * (s2 / c - x2);
    }
    dst[o] = x0;
    dst[o + 1] = x1;
    dst[o + 2] = x2;
}

__global__ __launch_bounds__(MC_BLOCK) void k_sm_copy(const float *__restrict__ src, float *__restrict__ dst, uint32_t V, SmPtr p) {
    if (p.hdr[H_FLAGS] & SM_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const uint64_t o = 3 * (uint64_t)v;
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[o + a] = src[o + a];
}

// ------------------------------------------------------------------------------------------------ normals
__global__ __launch_bounds__(MC_BLOCK) void k_sm_normals(const float *__restrict__ P, const float *__restrict__ nin,
                                                         const int32_t *__restrict__ fa, uint32_t V, SmPtr p, float *__restrict__ nout) {
    if (p.hdr[H_FLAGS] & SM_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    const uint32_t e = p.fend[v];
    for (uint32_t i = e - p.fdeg[v]; i < e; ++i) {
        const uint32_t g = p.flist[i];
        const uint64_t i0 = 3 * (uint64_t)mesh_fv(fa, g, 0), i1 = 3 * (uint64_t)mesh_fv(fa, g, 1), i2 = 3 * (uint64_t)mesh_fv(fa, g, 2);
        const float e1x = P[i1] - P[i0], e1y = P[i1 + 1] - P[i0 + 1], e1z = P[i1 + 2] - P[i0 + 2];
        const float e2x = P[i2] - P[i0], e2y = P[i2 + 1] - P[i0 + 1], e2z = P[i2 + 2] - P[i0 + 2];
        a0 += e1y * e2z - e1z * e2y;
        a1 += e1z * e2x - e1x * e2z;
        a2 += e1x * e2y - e1y * e2x;
    }
    const float q = a0 * a0 + a1 * a1 + a2 * a2;
    const uint64_t o = 3 * (uint64_t)v;
    if (q > 0.0f && q < __builtin_inff()) {
        const float r = sqrtf(q);
        nout[o] = a0 / r;
        nout[o + 1] = a1 / r;
        nout[o + 2] = a2 / r;
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) nout[o + a] = nin ? nin[o + a] : 0.0f;
    }
}

int sm_check(uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, SmPtr &p) {
    if (V >= (1u << 31) || F > SM_MAX_F) return CNERF_EINVAL;
    if (!ws) return CNERF_ENULL;
    return mesh_check_ws(ws, ws_bytes, sm_carve(ws, V, F, p));
}

}  // namespace

extern "C" {

int cnerf_mesh_smooth_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (V >= (1u << 31) || F > SM_MAX_F) return CNERF_EINVAL;
    if (!bytes_host) return CNERF_ENULL;
    SmPtr p;
    *bytes_host = sm_carve(nullptr, V, F, p);
    return CNERF_OK;
}

int cnerf_mesh_smooth_init(const int32_t *faces, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *flags, void *stream) {
    SmPtr p;
    if (const int rc = sm_check(V, F, ws, ws_bytes, p)) return rc;
    if ((F && !faces) || !flags) return CNERF_ENULL;
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(ws, 0, 256, st)) return rc;
    if (V) hipLaunchKernelGGL(k_sm_clear, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
    if (F) hipLaunchKernelGGL(k_sm_deg, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, p);
    if (V) {
        hipLaunchKernelGGL(k_sm_vsum, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
        hipLaunchKernelGGL(k_sm_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (uint32_t)cn_div_up64(V, MC_BLOCK), p);
        hipLaunchKernelGGL(k_sm_offsets, mesh_grid(V), dim3(MC_BLOCK), 0, st, V, p);
        if (F) hipLaunchKernelGGL(k_sm_fill, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, F, p);
    }
    hipLaunchKernelGGL(k_sm_sort, mesh_grid(V ? V : 1), dim3(MC_BLOCK), 0, st, V, p, flags);
    return cn_launch_status();
}

int cnerf_mesh_smooth_steps(const float *verts_in, uint32_t V, uint32_t F, uint32_t iterations, float lambda, float mu, int pin_boundary,
                            void *ws, uint64_t ws_bytes, float *verts_out, void *stream) {
    SmPtr p;
    if (const int rc = sm_check(V, F, ws, ws_bytes, p)) return rc;
    if (!__builtin_isfinite(lambda) || !__builtin_isfinite(mu)) return CNERF_EINVAL;
    if (V && (!verts_in || !verts_out)) return CNERF_ENULL;
    if (!V) return CNERF_OK;
    hipStream_t st = CN_STREAM(stream);
    const uint64_t per = mu != 0.0f ? 2 : 1, T = per * iterations;
    if (!T) {
        hipLaunchKernelGGL(k_sm_copy, mesh_grid(V), dim3(MC_BLOCK), 0, st, verts_in, verts_out, V, p);
        return cn_launch_status();
    }
    const float *src = verts_in;
    for (uint64_t t = 0; t < T; ++t) {
        float *dst = t + 1 == T ? verts_out : p.pos[t & 1];
        const float s = (t % per) ? mu : lambda;
        hipLaunchKernelGGL(k_sm_step, mesh_grid(V), dim3(MC_BLOCK), 0, st, src, dst, V, s, pin_boundary ? 1 : 0, p);
        src = dst;
    }
    return cn_launch_status();
}

int cnerf_mesh_smooth_normals(const float *verts, const float *normals_in, uint32_t V, const int32_t *faces, uint32_t F, void *ws,
                              uint64_t ws_bytes, float *normals_out, void *stream) {
    SmPtr p;
    if (const int rc = sm_check(V, F, ws, ws_bytes, p)) return rc;
    if (V && (!verts || !normals_out)) return CNERF_ENULL;
    if (F && !faces) return CNERF_ENULL;
    if (!V) return CNERF_OK;
    hipLaunchKernelGGL(k_sm_normals, mesh_grid(V), dim3(MC_BLOCK), 0, CN_STREAM(stream), verts, normals_in, faces, V, p, normals_out);
    return cn_launch_status();
}

}  // extern "C"
