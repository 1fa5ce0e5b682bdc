// Marching cubes over a dense float32 volume (cnerf_marching_cubes_*): count -> scan -> emit vertices -> emit faces, all on the caller's
// stream, no atomics, no host synchronisation.  Table and cube conventions: mc_tables.h / gen_mc_tables.py; the NumPy restatement the
// tests pin it to: tests/mc_restatement.py.
//
//   k_mc_count : one thread per grid point: the case of the cell whose minimum corner it is, the 3-bit mask of its crossing owned edges
//                (edge (p, p + e_axis) is owned by p); per-workgroup (vertex, triangle) totals by ballot / popcount + LDS
//   k_mc_scan  : one workgroup: exclusive scan of the workgroup totals (in place) and counts[2] = (vertices, triangles)
//   k_mc_verts : the in-workgroup prefix again (ballot + mbcnt, LDS wave totals); vertex base of every point, positions, normals
//   k_mc_faces : the same prefix over the triangle counts; each table edge -> owner point's base + rank of its axis in the owner's mask
//
// Vertices are ordered by (linear point index, axis), triangles by (linear cell index, table order): the output does not depend on
// scheduling.  Workspace: header (overflow flag) | case bytes [N] | mask bytes [N] | vertex bases uint32 [N] | workgroup totals uint2 [N/256].
#include "mesh_mc.h"            // the arithmetic and workspace regions shared with mesh_sparse.hip; mc_tables.h, mesh_common.h

namespace {

// the workspace of n grid points: its regions in order -> total bytes (ws == nullptr: the size only)
uint64_t mc_carve(void *ws, uint64_t n, McPtr &p) {
    MeshCarve c(ws);
    mc_take(c, n, p);
    return c.total();
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_count(const float *__restrict__ vol, uint32_t nx, uint32_t ny, uint32_t nz, float level,
                                                       uint8_t *__restrict__ cases, uint8_t *__restrict__ masks, uint2 *__restrict__ sums) {
    __shared__ uint32_t red_v[MC_WAVES], red_t[MC_WAVES];
    const uint32_t nyz = ny * nz, n = nx * nyz;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    uint32_t m = 0, ntri = 0;
    if (i < n) {
        const uint32_t x = i / nyz, r = i - x * nyz, y = r / nz, z = r - y * nz;
        const bool hx = x + 1 < nx, hy = y + 1 < ny, hz = z + 1 < nz;
        const bool in0 = mc_in(vol[i], level);
        if (hx && mc_in(vol[i + nyz], level) != in0) m |= 1u;
        if (hy && mc_in(vol[i + nz], level) != in0) m |= 2u;
        if (hz && mc_in(vol[i + 1], level) != in0) m |= 4u;
        uint32_t c = 0;
        if (hx && hy && hz) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t off = (k & 1 ? nyz : 0u) + (k & 2 ? nz : 0u) + (k & 4 ? 1u : 0u);
                c |= (uint32_t)mc_in(vol[i + off], level) << k;
            }
            ntri = cn_mc_ntri[c];
        }
        cases[i] = (uint8_t)c;
        masks[i] = (uint8_t)m;
    }
    const uint32_t tv = mc_block_total<2>((uint32_t)__popc(m), red_v);
    const uint32_t tt = mc_block_total<3>(ntri, red_t);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(tv, tt);
}

// one workgroup; sums[0..nblk) -> exclusive offsets in place; counts = totals, or 0xffffffff both (and flag = 1) when either exceeds INT32_MAX
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_mc_scan(uint2 *__restrict__ sums, uint32_t nblk, uint32_t *__restrict__ counts,
                                                           uint32_t *__restrict__ flag) {
    uint64_t cv, ct;
    mc_scan_totals(sums, nblk, cv, ct);
    if (threadIdx.x == 0) mc_store_counts(cv, ct, counts, flag);
}

// mc_grad's fetch for a dense volume: the value d steps of `stride` from point p
struct McDenseVal {
    const float *__restrict__ vol;
    uint32_t p, stride;
    __device__ __forceinline__ float operator()(int d) const { return d > 0 ? vol[p + stride] : d < 0 ? vol[p - stride] : vol[p]; }
};

__global__ __launch_bounds__(MC_BLOCK) void k_mc_verts(const float *__restrict__ vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, McGeom g,
                                                       const uint8_t *__restrict__ masks, const uint2 *__restrict__ sums,
                                                       const uint32_t *__restrict__ flag, uint32_t *__restrict__ vbase, float *__restrict__ verts,
                                                       float *__restrict__ normals, uint32_t max_verts) {
    __shared__ uint32_t red[MC_WAVES];
    if (flag[0]) return;                             // the totals overflowed int32: nothing is written
    const uint32_t nyz = ny * nz, n = nx * nyz;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t m = i < n ? masks[i] : 0u;
    const uint32_t base = sums[blockIdx.x].x + mc_block_prefix<2>((uint32_t)__popc(m), red);
    if (i >= n) return;
    vbase[i] = base;
    if (!m) return;
    const uint32_t x = i / nyz, r = i - x * nyz, y = r / nz, z = r - y * nz;
    const uint32_t idx[3] = {x, y, z}, len[3] = {nx, ny, nz}, stride[3] = {nyz, nz, 1u};
    const float v0 = vol[i];
    uint32_t vid = base;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((m >> a) & 1u)) continue;
        const uint32_t j = i + stride[a];
        if (vid < max_verts) {
            const float t = mc_cross_t(level, v0, vol[j]);
            float p[3];
            mc_vertex_pos(g, idx, a, t, p);
            const uint64_t o = 3 * (uint64_t)vid;
            verts[o] = p[0];
            verts[o + 1] = p[1];
            verts[o + 2] = p[2];
            if (normals) {
                float g0[3], g1[3], nv[3];
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const uint32_t jb = b == a ? idx[b] + 1 : idx[b];
                    g0[b] = mc_grad(McDenseVal{vol, i, stride[b]}, idx[b], len[b], g.sp[b]);
                    g1[b] = mc_grad(McDenseVal{vol, j, stride[b]}, jb, len[b], g.sp[b]);
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

__global__ __launch_bounds__(MC_BLOCK) void k_mc_faces(uint32_t nx, uint32_t ny, uint32_t nz, const uint8_t *__restrict__ cases,
                                                       const uint8_t *__restrict__ masks, const uint2 *__restrict__ sums,
                                                       const uint32_t *__restrict__ flag, const uint32_t *__restrict__ vbase,
                                                       int32_t *__restrict__ faces, uint32_t max_faces) {
    __shared__ uint32_t red[MC_WAVES];
    if (flag[0]) return;
    const uint32_t nyz = ny * nz, n = nx * nyz;
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t c = i < n ? cases[i] : 0u;
    const uint32_t nt = cn_mc_ntri[c];               // 0 for the points that own no cell (their case byte is 0)
    const uint32_t base = sums[blockIdx.x].y + mc_block_prefix<3>(nt, red);
    for (uint32_t k = 0; k < nt; ++k) {
        const uint32_t f = base + k;
        if (f >= max_faces) break;
        int32_t tri[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            uint32_t corner, axis;
            mc_edge_owner((uint32_t)cn_mc_tri[c][3 * k + q], corner, axis);
            const uint32_t owner = i + (corner & 1u ? nyz : 0u) + (corner & 2u ? nz : 0u) + (corner & 4u ? 1u : 0u);
            tri[q] = mc_vertex_id(vbase[owner], masks[owner], axis);
        }
        const uint64_t o = 3 * (uint64_t)f;
        faces[o] = tri[0];
        faces[o + 1] = tri[1];
        faces[o + 2] = tri[2];
    }
}

int mc_check_dims(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return CNERF_EINVAL;
    if ((uint64_t)nx * ny * nz >= (1ull << 31)) return CNERF_EINVAL;
    return CNERF_OK;
}

}  // namespace

extern "C" {

int cnerf_marching_cubes_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t *bytes_host) {
    if (const int rc = mc_check_dims(nx, ny, nz)) return rc;
    if (!bytes_host) return CNERF_ENULL;
    McPtr p;
    *bytes_host = mc_carve(nullptr, (uint64_t)nx * ny * nz, p);
    return CNERF_OK;
}

int cnerf_marching_cubes_count(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void *ws, uint64_t ws_bytes,
                               uint32_t *counts, void *stream) {
    if (const int rc = mc_check_dims(nx, ny, nz)) return rc;
    if (!vol || !ws || !counts) return CNERF_ENULL;
    const uint32_t n = nx * ny * nz;
    McPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, mc_carve(ws, n, p))) return rc;
    hipLaunchKernelGGL(k_mc_count, mesh_grid(n), dim3(MC_BLOCK), 0, CN_STREAM(stream), vol, nx, ny, nz, level, p.cases, p.masks, p.sums);
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, CN_STREAM(stream), p.sums, cn_div_up(n, MC_BLOCK), counts, p.flag);
    return cn_launch_status();
}

int cnerf_marching_cubes_emit(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const float *origin_host,
                              const float *spacing_host, void *ws, uint64_t ws_bytes, float *verts, float *normals, int32_t *faces,
                              uint32_t max_verts, uint32_t max_faces, void *stream) {
    if (const int rc = mc_check_dims(nx, ny, nz)) return rc;
    if (!vol || !origin_host || !spacing_host || !ws || (max_verts && !verts) || (max_faces && !faces)) return CNERF_ENULL;
    const uint32_t n = nx * ny * nz;
    McPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, mc_carve(ws, n, p))) return rc;
    const McGeom g = mc_geom(origin_host, spacing_host);
    hipLaunchKernelGGL(k_mc_verts, mesh_grid(n), dim3(MC_BLOCK), 0, CN_STREAM(stream), vol, nx, ny, nz, level, g, (const uint8_t *)p.masks,
                       (const uint2 *)p.sums, (const uint32_t *)p.flag, p.vbase, verts, max_verts ? normals : nullptr, max_verts);
    hipLaunchKernelGGL(k_mc_faces, mesh_grid(n), dim3(MC_BLOCK), 0, CN_STREAM(stream), nx, ny, nz, (const uint8_t *)p.cases,
                       (const uint8_t *)p.masks, (const uint2 *)p.sums, (const uint32_t *)p.flag, (const uint32_t *)p.vbase, faces,
                       max_faces);
    return cn_launch_status();
}

}  // extern "C"
