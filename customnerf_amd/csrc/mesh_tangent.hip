// Welded vertices and tangent frames of a UV-mapped mesh on the device (cnerf_mesh_tangent_*), what a tangent-space normal map and a glTF
// primitive need: face corners with the same (vertex, u, v) become one output vertex, every output vertex gets a tangent and a handedness
// from the faces around it, and the per-vertex arrays are gathered.  Same conventions as mesh_smooth.hip: the caller's stream and workspace,
// no allocation, no host sync; counts (W and the flags) is the one host read.  The only atomics are integer ones whose result does not
// depend on their order (degrees, list slots, the flag bit): every list is sorted before anything reads it, every sum runs in ascending
// corner index, so the output is bit-reproducible and tests/tangent_restatement.py restates it bit for bit.  The rules are in
// include/customnerf_hip.h.
//
// Workspace: header | per vertex: corner count, list end, group count, first output vertex | workgroup totals | corner lists u32 [3F] |
//   group rank of every list entry u32 [3F] | group normals float32 [3F][3].
//
// weld:
//   k_tg_deg                            : per face: index check (flags bit 0), corner counts (atomicAdd)
//   k_tg_vsum / k_tg_scan / k_tg_offsets : exclusive scan of a per-vertex counter (mesh_common.h); run twice: corners, then groups
//   k_tg_fill                           : per face: its corners into their vertices' lists (atomicAdd on the list ends)
//   k_tg_group                          : per vertex: the list sorted; every entry gets the rank of its group, a group being the entries
//                                         with the same UV bits, ranked by their first entry
//   k_tg_emit                           : per vertex: corner_vertex of its corners, vertex_corner of its groups; counts out
// frames  : k_tg_frames per vertex, for each of its groups: the sums over the group's corners, the frame, written to every corner
// vertices: k_tg_vertices per output vertex and corner: the gather
#include "common.h"
#include "mesh_common.h"

#define TG_BAD_INDEX 1u
#define TG_MAX_F 0x2AAAAAAAu                         // 3 F corners fit an int32

namespace {

enum { H_FLAGS = 0, H_W = 1 };                       // uint32 slots of the header

struct TgPtr {
    uint32_t *hdr, *deg, *end, *gcnt, *gbase;
    uint2 *sums;
    uint32_t *list, *grp;
    float *gnorm;
};

uint64_t tg_carve(void *ws, uint64_t V, uint64_t F, TgPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.deg = c.take<uint32_t>(V);
    p.end = c.take<uint32_t>(V);
    p.gcnt = c.take<uint32_t>(V);
    p.gbase = c.take<uint32_t>(V);
    p.sums = c.take<uint2>(cn_div_up64(V ? V : 1, MC_BLOCK));
    p.list = c.take<uint32_t>(3 * F);
    p.grp = c.take<uint32_t>(3 * F);
    p.gnorm = c.take<float>(9 * F);
    return c.total();
}

// ------------------------------------------------------------------------------------------------ weld
__global__ __launch_bounds__(MC_BLOCK) void k_tg_deg(const int32_t *__restrict__ fa, uint32_t V, uint32_t F, TgPtr p) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    if (!mesh_face(fa, f, V, t)) {
        atomicOr(p.hdr + H_FLAGS, TG_BAD_INDEX);
        return;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) atomicAdd(p.deg + t[q], 1u);
}

// the scan of cnt [V] into out [V]: workgroup totals, their offsets (and the total into hdr[slot] when slot >= 0), the starts
__global__ __launch_bounds__(MC_BLOCK) void k_tg_vsum(uint32_t V, const uint32_t *__restrict__ cnt, TgPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    mesh_csr_totals(v < V ? cnt[v] : 0, 0, p.sums);
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_tg_scan(uint32_t nblk, int slot, TgPtr p) {
    uint64_t c, z;
    mc_scan_totals(p.sums, nblk, c, z);              // at most 3 F < 2^32
    if (slot >= 0 && threadIdx.x == 0) p.hdr[slot] = (uint32_t)c;
}

__global__ __launch_bounds__(MC_BLOCK) void k_tg_offsets(uint32_t V, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ out, TgPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t s = mesh_csr_start(p.sums[blockIdx.x].x, v < V ? cnt[v] : 0, red);
    if (v < V) out[v] = s;
}

__global__ __launch_bounds__(MC_BLOCK) void k_tg_fill(const int32_t *__restrict__ fa, uint32_t F, TgPtr p) {
    if (p.hdr[H_FLAGS] & TG_BAD_INDEX) return;
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) p.list[atomicAdd(p.end + mesh_fv(fa, f, q), 1u)] = 3 * f + q;   // k_tg_fill ends at start + degree
}

// the bit patterns of corner c's UV: -0 is not +0, a NaN equals itself
__device__ __forceinline__ uint2 tg_uv_bits(const float *__restrict__ uvs, uint32_t c) {
    return make_uint2(__float_as_uint(uvs[2 * (uint64_t)c]), __float_as_uint(uvs[2 * (uint64_t)c + 1]));
}

__global__ __launch_bounds__(MC_BLOCK) void k_tg_group(const float *__restrict__ uvs, uint32_t V, TgPtr p) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    if (p.hdr[H_FLAGS] & TG_BAD_INDEX) {
        p.gcnt[v] = 0;
        return;
    }
    const uint32_t d = p.deg[v], start = p.end[v] - d;
    uint32_t *l = p.list + start, *g = p.grp + start;
    mesh_isort(l, d);
    uint32_t n = 0;
    for (uint32_t i = 0; i < d; ++i) {
        const uint2 k = tg_uv_bits(uvs, l[i]);
        uint32_t r = n;
        for (uint32_t j = 0; j < i; ++j) {
            const uint2 o = tg_uv_bits(uvs, l[j]);
            if (o.x == k.x && o.y == k.y) {
                r = g[j];
                break;
            }
        }
        g[i] = r;
        n += r == n;
    }
    p.gcnt[v] = n;
}

__global__ __launch_bounds__(MC_BLOCK) void k_tg_emit(uint32_t V, TgPtr p, uint32_t *__restrict__ counts, int32_t *__restrict__ corner_vertex,
                                                      uint32_t max_faces, int32_t *__restrict__ vertex_corner, uint32_t max_verts) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    const bool bad = p.hdr[H_FLAGS] & TG_BAD_INDEX;
    if (v == 0) {
        counts[0] = bad ? 0u : p.hdr[H_W];
        counts[1] = p.hdr[H_FLAGS];
    }
    if (v >= V || bad) return;
    const uint32_t d = p.deg[v], start = p.end[v] - d, base = p.gbase[v];
    uint32_t seen = 0;
    for (uint32_t i = 0; i < d; ++i) {
        const uint32_t c = p.list[start + i], r = p.grp[start + i], w = base + r;
        if (c / 3 < max_faces) corner_vertex[c] = (int32_t)w;
        if (r == seen) {                             // the group's first, i.e. smallest, corner
            if (w < max_verts) vertex_corner[w] = (int32_t)c;
            ++seen;
        }
    }
}

// ------------------------------------------------------------------------------------------------ frames
__device__ __forceinline__ double tg_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ bool tg_pos(double x) { return x > 0.0 && x < (double)INFINITY; }

// What face f gives each of its corners: A2 Tf / |Tf|, A2 Bf / |Bf| and e1 x e2; false for a face that contributes nothing
__device__ __forceinline__ bool tg_face(const float *__restrict__ verts, const int32_t *__restrict__ fa, const float *__restrict__ uvs, uint32_t f,
                                        double cT[3], double cB[3], double cN[3]) {
    float p0[3], p1[3], p2[3];
    at_load3(verts, mesh_fv(fa, f, 0), p0);
    at_load3(verts, mesh_fv(fa, f, 1), p1);
    at_load3(verts, mesh_fv(fa, f, 2), p2);
    const float *uv = uvs + 6 * (uint64_t)f;
    const double du1 = (double)(uv[2] - uv[0]), dv1 = (double)(uv[3] - uv[1]), du2 = (double)(uv[4] - uv[0]), dv2 = (double)(uv[5] - uv[1]);
    double e1[3], e2[3], T[3], B[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = (double)(p1[k] - p0[k]);
        e2[k] = (double)(p2[k] - p0[k]);
    }
    const double det = du1 * dv2 - du2 * dv1;
    if (!(det != 0.0) || !(fabs(det) < (double)INFINITY)) return false;
    const double s = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T[k] = s * (e1[k] * dv2 - e2[k] * dv1);
        B[k] = s * (e2[k] * du1 - e1[k] * du2);
    }
    cN[0] = e1[1] * e2[2] - e1[2] * e2[1];
    cN[1] = e1[2] * e2[0] - e1[0] * e2[2];
    cN[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double A2 = sqrt(tg_dot(cN, cN)), lT = sqrt(tg_dot(T, T)), lB = sqrt(tg_dot(B, B));
    if (!tg_pos(A2) || !tg_pos(lT) || !tg_pos(lB)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cT[k] = (A2 * T[k]) / lT;
        cB[k] = (A2 * B[k]) / lB;
    }
    return true;
}

__global__ __launch_bounds__(MC_BLOCK) void k_tg_frames(const float *__restrict__ verts, const int32_t *__restrict__ fa,
                                                        const float *__restrict__ uvs, const float *__restrict__ normals, uint32_t V, TgPtr p,
                                                        float *__restrict__ tangents, uint32_t max_faces) {
    if (p.hdr[H_FLAGS] & TG_BAD_INDEX) return;
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const uint32_t d = p.deg[v], start = p.end[v] - d, ng = p.gcnt[v], base = p.gbase[v];
    const uint32_t *l = p.list + start, *g = p.grp + start;
    for (uint32_t r = 0; r < ng; ++r) {
        double ST[3] = {0.0, 0.0, 0.0}, SB[3] = {0.0, 0.0, 0.0}, SN[3] = {0.0, 0.0, 0.0};
        for (uint32_t i = 0; i < d; ++i) {
            if (g[i] != r) continue;
            double cT[3], cB[3], cN[3];
            if (!tg_face(verts, fa, uvs, l[i] / 3, cT, cB, cN)) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ST[k] += cT[k];
                SB[k] += cB[k];
                SN[k] += cN[k];
            }
        }
        double n[3] = {SN[0], SN[1], SN[2]};
        if (normals) {
            float nf[3];
            at_load3(normals, v, nf);
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = (double)nf[k];
        }
        const double qn = tg_dot(n, n);
        if (tg_pos(qn)) {
            const double ln = sqrt(qn);
#pragma unroll
            for (int k = 0; k < 3; ++k) n[k] = n[k] / ln;
        } else {
            n[0] = n[1] = n[2] = 0.0;                // unusable: the fallback's axis is then x and t = (1, 0, 0)
        }
        double t[3];
        const double nT = tg_dot(n, ST);
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = ST[k] - n[k] * nT;
        double q = tg_dot(t, t);
        if (!(q >= __DBL_MIN__ && q < (double)INFINITY)) {
            int a = 0;
            if (fabs(n[1]) < fabs(n[a])) a = 1;
            if (fabs(n[2]) < fabs(n[a])) a = 2;
            const double na = n[a];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = (k == a ? 1.0 : 0.0) - n[k] * na;
            q = tg_dot(t, t);
        }
        const double lt = sqrt(q);
        const double x[3] = {n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]};
        const float out[4] = {(float)(t[0] / lt), (float)(t[1] / lt), (float)(t[2] / lt), tg_dot(x, SB) < 0.0 ? -1.0f : 1.0f};
        float *gn = p.gnorm + 3 * (uint64_t)(base + r);
#pragma unroll
        for (int k = 0; k < 3; ++k) gn[k] = (float)n[k];
        for (uint32_t i = 0; i < d; ++i) {
            if (g[i] != r || l[i] / 3 >= max_faces) continue;
            float *o = tangents + 4 * (uint64_t)l[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = out[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ vertices
__global__ __launch_bounds__(MC_BLOCK) void k_tg_vertices(const float *__restrict__ verts, const int32_t *__restrict__ fa,
                                                          const float *__restrict__ uvs, const float *__restrict__ normals,
                                                          const float *__restrict__ tangents, const int32_t *__restrict__ corner_vertex,
                                                          const int32_t *__restrict__ vertex_corner, uint32_t F, uint32_t W, TgPtr p,
                                                          float *__restrict__ pos, float *__restrict__ nrm, float *__restrict__ uvo,
                                                          float *__restrict__ tan, uint32_t *__restrict__ indices) {
    if (p.hdr[H_FLAGS] & TG_BAD_INDEX) return;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i < 3 * F) indices[i] = (uint32_t)corner_vertex[i];
    if (i >= W || i >= p.hdr[H_W]) return;
    const uint32_t c = (uint32_t)vertex_corner[i];
    if (c >= 3 * F) return;
    const uint32_t v = mesh_fv(fa, c / 3, c % 3);    // weld checked the faces
    float a[3];
    at_load3(verts, v, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[3 * (uint64_t)i + k] = a[k];
    at_load3(normals ? normals : p.gnorm, normals ? v : i, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[3 * (uint64_t)i + k] = a[k];
    uvo[2 * (uint64_t)i] = uvs[2 * (uint64_t)c];
    uvo[2 * (uint64_t)i + 1] = 1.0f - uvs[2 * (uint64_t)c + 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) tan[4 * (uint64_t)i + k] = tangents[4 * (uint64_t)c + k];
}

int tg_check(uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, TgPtr &p) {
    if (V >= (1u << 31) || F > TG_MAX_F) return CNERF_EINVAL;
    if (!ws) return CNERF_ENULL;
    return mesh_check_ws(ws, ws_bytes, tg_carve(ws, V, F, p));
}

}  // namespace

extern "C" {

int cnerf_mesh_tangent_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (V >= (1u << 31) || F > TG_MAX_F) return CNERF_EINVAL;
    if (!bytes_host) return CNERF_ENULL;
    TgPtr p;
    *bytes_host = tg_carve(nullptr, V, F, p);
    return CNERF_OK;
}

int cnerf_mesh_tangent_weld(const int32_t *faces, const float *uvs, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts,
                            int32_t *corner_vertex, uint32_t max_faces, int32_t *vertex_corner, uint32_t max_verts, void *stream) {
    TgPtr p;
    if (const int rc = tg_check(V, F, ws, ws_bytes, p)) return rc;
    if (!counts || (F && (!faces || !uvs)) || (F && max_faces && !corner_vertex) || (F && max_verts && !vertex_corner)) return CNERF_ENULL;
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(ws, 0, 256, st)) return rc;
    if (V) {
        if (const int rc = (int)hipMemsetAsync(p.deg, 0, sizeof(uint32_t) * (uint64_t)V, st)) return rc;
    }
    if (F) hipLaunchKernelGGL(k_tg_deg, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, p);
    if (V) {
        const dim3 grid = mesh_grid(V);
        hipLaunchKernelGGL(k_tg_vsum, grid, dim3(MC_BLOCK), 0, st, V, p.deg, p);
        hipLaunchKernelGGL(k_tg_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, grid.x, -1, p);
        hipLaunchKernelGGL(k_tg_offsets, grid, dim3(MC_BLOCK), 0, st, V, p.deg, p.end, p);
        if (F) hipLaunchKernelGGL(k_tg_fill, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, F, p);
        hipLaunchKernelGGL(k_tg_group, grid, dim3(MC_BLOCK), 0, st, uvs, V, p);
        hipLaunchKernelGGL(k_tg_vsum, grid, dim3(MC_BLOCK), 0, st, V, p.gcnt, p);
        hipLaunchKernelGGL(k_tg_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, grid.x, (int)H_W, p);
        hipLaunchKernelGGL(k_tg_offsets, grid, dim3(MC_BLOCK), 0, st, V, p.gcnt, p.gbase, p);
    }
    hipLaunchKernelGGL(k_tg_emit, mesh_grid(V ? V : 1), dim3(MC_BLOCK), 0, st, V, p, counts, corner_vertex, max_faces, vertex_corner, max_verts);
    return cn_launch_status();
}

int cnerf_mesh_tangent_frames(const float *verts, const int32_t *faces, const float *uvs, const float *normals, uint32_t V, uint32_t F,
                              void *ws, uint64_t ws_bytes, float *tangents, uint32_t max_faces, void *stream) {
    TgPtr p;
    if (const int rc = tg_check(V, F, ws, ws_bytes, p)) return rc;
    if (!F || !V || !max_faces) return CNERF_OK;
    if (!verts || !faces || !uvs || !tangents) return CNERF_ENULL;
    hipLaunchKernelGGL(k_tg_frames, mesh_grid(V), dim3(MC_BLOCK), 0, CN_STREAM(stream), verts, faces, uvs, normals, V, p, tangents, max_faces);
    return cn_launch_status();
}

int cnerf_mesh_tangent_vertices(const float *verts, const int32_t *faces, const float *uvs, const float *normals, const float *tangents,
                                const int32_t *corner_vertex, const int32_t *vertex_corner, uint32_t V, uint32_t F, uint32_t W, void *ws,
                                uint64_t ws_bytes, float *positions, float *normals_out, float *uvs_out, float *tangents_out,
                                uint32_t *indices, void *stream) {
    TgPtr p;
    if (const int rc = tg_check(V, F, ws, ws_bytes, p)) return rc;
    if ((uint64_t)W > 3 * (uint64_t)F) return CNERF_EINVAL;
    if (!F) return CNERF_OK;
    if (!verts || !faces || !uvs || !tangents || !corner_vertex || !indices) return CNERF_ENULL;
    if (W && (!vertex_corner || !positions || !normals_out || !uvs_out || !tangents_out)) return CNERF_ENULL;
    hipLaunchKernelGGL(k_tg_vertices, mesh_grid(3 * (uint64_t)F), dim3(MC_BLOCK), 0, CN_STREAM(stream), verts, faces, uvs, normals, tangents,
                       corner_vertex, vertex_corner, F, W, p, positions, normals_out, uvs_out, tangents_out, indices);
    return cn_launch_status();
}

}  // extern "C"
