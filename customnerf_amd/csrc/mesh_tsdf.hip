// TSDF fusion of depth maps on marching cubes' lattice (cnerf_tsdf_*): the surface that a set of rendered or rasterised views shows, as
// the zero level of a float32 volume that cnerf_marching_cubes_* meshes.  Same conventions as the other mesh passes: the caller's stream
// and buffers, no allocation, no host synchronisation, no float atomics.  The rules are in include/customnerf_hip.h; the NumPy restatement
// the tests pin them to: tests/tsdf_restatement.py.
//
//   k_tsdf_integrate : one thread per two z-adjacent lattice points: their (acc, weight) pairs are read once (16 bytes), the launch's views
//                      (at most TSDF_BATCH, passed by value: wave-uniform, so the cameras sit in scalar registers) are walked in index
//                      order with the sums in registers, and the pairs are written once.  A point's sums run in view order whatever
//                      the cut into launches.  A workgroup owns a brick of points, not a run of the z axis (below)
//   k_tsdf_finalize  : one thread per point: acc / weight or the fill value; observed points counted by ballot, one integer add per wave
//   k_tsdf_face_keep : one thread per face: the cell that holds its centroid has eight observed corners
//
// The camera is the rasteriser's (mesh_camera.h), so a point lands in the pixel whose depth mesh.rasterize or a renderer wrote.
#include "mesh_camera.h"
#include "mesh_mc.h"            // McGeom / mc_geom: the lattice's origin and spacing as marching cubes takes them

#define TSDF_BATCH 16
#define TSDF_UNROLL 4                                            // divides TSDF_BATCH

namespace {

struct TsdfViews {
    MeshCam cam[TSDF_BATCH];
    uint32_t n;                                                  // views of this launch
};

// One view's say about the point p in two halves, so that the pixel reads of TSDF_UNROLL views are in flight together: steps 1-8 of the
// header's rule give the pixel (ok: the point projects into the image; pix = 0 otherwise, a pixel that exists) and the distance r ...
__device__ __forceinline__ bool tsdf_pixel(const MeshCam &cam, const float p[3], uint32_t H, uint32_t W, int depth_kind, uint32_t &pix,
                                           float &r) {
    const float d0 = p[0] - cam.m[0][3], d1 = p[1] - cam.m[1][3], d2 = p[2] - cam.m[2][3];
    float z, X, Y;
    mesh_cam_project(cam, d0, d1, d2, z, X, Y);
    bool ok = z >= cam.near;                                     // false behind the camera, nearer than near, or for a NaN
    ok = ok && X >= 0.0f && X < (float)W && Y >= 0.0f && Y < (float)H;
    const uint32_t ix = ok ? (uint32_t)(int)floorf(X) : 0u, iy = ok ? (uint32_t)(int)floorf(Y) : 0u;
    ok = ok && ix < W && iy < H;                                 // (float) W rounded up: only for W, H > 2^24
    pix = ok ? iy * W + ix : 0u;                                 // H W < 2^31
    r = depth_kind == 0 ? z : sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    return ok;
}

// ... and steps 9-14 add the pixel's depth D and weight w to the point's sums
__device__ __forceinline__ void tsdf_add(bool ok, float D, float w, float r, float trunc, float2 &s) {
    const float sdf = D - r;
    ok = ok && D > 0.0f && w > 0.0f && w < INFINITY && !(sdf < -trunc);   // NaN, 0, negative depth or weight: nothing; behind the surface: hidden
    const float sv = -fminf(1.0f, sdf / trunc);
    if (ok) {
        s.x += w * sv;
        s.y += w;
    }
}

// A workgroup owns a brick of 4 x 4 x 32 points and a wave a 4 x 4 x 8 part of it: lane = (x 4 + y) 4 + z / 2.  A wave's points project
// into a patch of a few pixels a side, so one pixel read touches a handful of cache lines; 64 points along z touch up to 64, and 16 views
// of 512 x 512 then ran at a third of this speed (docs/HISTORY.md B.26).  A row of 16 points along z is one 128-byte line of the state.
#define TSDF_BX 4
#define TSDF_BY 4
#define TSDF_BZ 32

__global__ __launch_bounds__(MC_BLOCK) void k_tsdf_integrate(float2 *__restrict__ state, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t by,
                                                             uint32_t bz, McGeom g, TsdfViews vs, const float *__restrict__ depth,
                                                             const float *__restrict__ pixel_weight, uint32_t H, uint32_t W, float trunc,
                                                             int depth_kind) {
    const uint32_t bx_i = blockIdx.x / (by * bz), br = blockIdx.x - bx_i * (by * bz), by_i = br / bz, bz_i = br - by_i * bz;
    const uint32_t lane = cn_lane(), wave = threadIdx.x / CN_WAVE;
    const uint32_t x = bx_i * TSDF_BX + (lane >> 4), y = by_i * TSDF_BY + ((lane >> 2) & 3u);
    const uint32_t z0 = bz_i * TSDF_BZ + wave * 8u + (lane & 3u) * 2u;
    if (x >= nx || y >= ny || z0 >= nz) return;
    const uint32_t i0 = (x * ny + y) * nz + z0;                  // < 2^31
    const bool pair = z0 + 1 < nz, wide = pair && !(i0 & 1u);    // pair: the second point exists; wide: one aligned 16-byte access
    float2 s[2];
    if (wide) {
        const float4 t = *(const float4 *)(state + i0);
        s[0] = make_float2(t.x, t.y);
        s[1] = make_float2(t.z, t.w);
    } else {
        s[0] = state[i0];
        s[1] = pair ? state[i0 + 1] : make_float2(0.0f, 0.0f);
    }
    float p[2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {                                // without a second point the first one stands in; its sums are dropped
        p[j][0] = g.org[0] + (float)x * g.sp[0];
        p[j][1] = g.org[1] + (float)y * g.sp[1];
        p[j][2] = g.org[2] + (float)(z0 + (pair ? j : 0)) * g.sp[2];
    }
    const uint64_t HW = (uint64_t)H * W;
    for (uint32_t v0 = 0; v0 < vs.n; v0 += TSDF_UNROLL) {        // vs.n is uniform
        bool ok[TSDF_UNROLL][2];
        float r[TSDF_UNROLL][2], D[TSDF_UNROLL][2], w[TSDF_UNROLL][2];
#pragma unroll
        for (int u = 0; u < TSDF_UNROLL; ++u) {
            const bool live = v0 + u < vs.n;                     // uniform
            const uint64_t px0 = (v0 + u) * HW;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ok[u][j] = false;
                r[u][j] = D[u][j] = w[u][j] = 0.0f;
                if (live) {
                    uint32_t pix;
                    ok[u][j] = tsdf_pixel(vs.cam[v0 + u], p[j], H, W, depth_kind, pix, r[u][j]);
                    D[u][j] = depth[px0 + pix];
                    w[u][j] = pixel_weight ? pixel_weight[px0 + pix] : 1.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < TSDF_UNROLL; ++u) {                  // in view order
#pragma unroll
            for (int j = 0; j < 2; ++j) tsdf_add(ok[u][j], D[u][j], w[u][j], r[u][j], trunc, s[j]);
        }
    }
    if (wide) {
        *(float4 *)(state + i0) = make_float4(s[0].x, s[0].y, s[1].x, s[1].y);
    } else {
        state[i0] = s[0];
        if (pair) state[i0 + 1] = s[1];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_tsdf_finalize(const float2 *__restrict__ state, uint32_t n, float fill,
                                                            float *__restrict__ volume, uint32_t *__restrict__ observed) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    bool seen = false;
    if (i < n) {
        const float2 s = state[i];
        seen = s.y > 0.0f;
        volume[i] = seen ? s.x / s.y : fill;
    }
    const uint64_t b = __ballot(seen);
    if (b && cn_lane() == (uint32_t)__ffsll((unsigned long long)b) - 1) atomicAdd(observed, (uint32_t)__popcll(b));   // integer: any order
}

__global__ __launch_bounds__(MC_BLOCK) void k_tsdf_face_keep(const float2 *__restrict__ state, uint32_t nx, uint32_t ny, uint32_t nz,
                                                             McGeom g, const float *__restrict__ verts, uint32_t V,
                                                             const int32_t *__restrict__ faces, uint32_t F, uint8_t *__restrict__ keep) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    uint32_t t[3];
    bool ok = mesh_face(faces, f, V, t);
    if (ok) {
        const uint32_t len[3] = {nx, ny, nz};
        uint32_t q[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float c = ((verts[3 * (uint64_t)t[0] + b] + verts[3 * (uint64_t)t[1] + b]) + verts[3 * (uint64_t)t[2] + b]) / 3.0f;
            const float k = floorf((c - g.org[b]) / g.sp[b]);
            q[b] = (uint32_t)fminf(fmaxf(k, 0.0f), (float)(len[b] - 2));          // the clamp first: NaN -> 0, and the cast stays in range
        }
        const uint32_t base = (q[0] * ny + q[1]) * nz + q[2];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t o = base + ((k & 1 ? ny : 0u) + (k & 2 ? 1u : 0u)) * nz + (k & 4 ? 1u : 0u);
            ok &= state[o].y > 0.0f;
        }
    }
    keep[f] = ok ? 1 : 0;
}

// every extent >= 2 and at most 2^31 points
bool tsdf_dims_ok(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return false;
    const uint64_t xy = (uint64_t)nx * ny;                       // < 2^64
    return xy <= (1ull << 31) && xy * nz <= (1ull << 31);
}

}  // namespace

extern "C" {

int cnerf_tsdf_integrate(float *state, uint32_t nx, uint32_t ny, uint32_t nz, const float *origin_host, const float *spacing_host, float trunc,
                         const float *depth, const float *pixel_weight, uint32_t n_views, uint32_t H, uint32_t W, const float *c2w_host,
                         float fx, float fy, float cx, float cy, int convention, float near, int depth_kind, void *stream) {
    if (!tsdf_dims_ok(nx, ny, nz) || !(trunc > 0.0f && trunc < INFINITY) || !mesh_cam_ok(fx, fy, cx, cy, near, convention) ||
        depth_kind < 0 || depth_kind > 1 || (uint64_t)H * W >= (1ull << 31))
        return CNERF_EINVAL;
    if (!n_views) return CNERF_OK;
    if (!state || !depth || !c2w_host || !origin_host || !spacing_host) return CNERF_ENULL;
    const uint64_t HW = (uint64_t)H * W;
    if (!HW) return CNERF_OK;                                    // no pixel: no point projects into the image
    const McGeom g = mc_geom(origin_host, spacing_host);
    const uint32_t by = cn_div_up(ny, TSDF_BY), bz = cn_div_up(nz, TSDF_BZ);
    const dim3 grid((uint32_t)((uint64_t)cn_div_up(nx, TSDF_BX) * by * bz));     // <= 2^28: ceil(a / k) <= a / 2 for a >= 2
    for (uint32_t b = 0; b < n_views; b += TSDF_BATCH) {
        TsdfViews vs;
        vs.n = n_views - b < TSDF_BATCH ? n_views - b : TSDF_BATCH;
        for (uint32_t v = 0; v < TSDF_BATCH; ++v)                 // the slots past vs.n repeat the last view and are never read
            vs.cam[v] = mesh_cam(c2w_host + 12 * (uint64_t)(b + (v < vs.n ? v : vs.n - 1)), fx, fy, cx, cy, near, convention);
        hipLaunchKernelGGL(k_tsdf_integrate, grid, dim3(MC_BLOCK), 0, CN_STREAM(stream), (float2 *)state, nx, ny, nz, by, bz, g, vs,
                           depth + b * HW, pixel_weight ? pixel_weight + b * HW : nullptr, H, W, trunc, depth_kind);
    }
    return cn_launch_status();
}

int cnerf_tsdf_finalize(const float *state, uint32_t nx, uint32_t ny, uint32_t nz, float fill, float *volume, uint32_t *observed, void *stream) {
    if (!tsdf_dims_ok(nx, ny, nz)) return CNERF_EINVAL;
    if (!state || !volume || !observed) return CNERF_ENULL;
    const uint32_t n = (uint32_t)((uint64_t)nx * ny * nz);
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(observed, 0, sizeof(uint32_t), st)) return rc;
    hipLaunchKernelGGL(k_tsdf_finalize, mesh_grid(n), dim3(MC_BLOCK), 0, st, (const float2 *)state, n, fill, volume, observed);
    return cn_launch_status();
}

int cnerf_tsdf_face_keep(const float *state, uint32_t nx, uint32_t ny, uint32_t nz, const float *origin_host, const float *spacing_host,
                         const float *verts, uint32_t V, const int32_t *faces, uint32_t F, uint8_t *keep, void *stream) {
    if (!tsdf_dims_ok(nx, ny, nz) || V >= (1u << 31) || F >= (1u << 31)) return CNERF_EINVAL;
    if (!F) return CNERF_OK;
    if (!state || !origin_host || !spacing_host || !faces || !keep || (V && !verts)) return CNERF_ENULL;
    hipLaunchKernelGGL(k_tsdf_face_keep, mesh_grid(F), dim3(MC_BLOCK), 0, CN_STREAM(stream), (const float2 *)state, nx, ny, nz,
                       mc_geom(origin_host, spacing_host), verts, V, faces, F, keep);
    return cn_launch_status();
}

}  // extern "C"
