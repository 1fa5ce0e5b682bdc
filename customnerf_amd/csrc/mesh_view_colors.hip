// Multi-view colour fusion (cnerf_view_colors_*): the colour of surface points — the texels of a bake, the vertices of a mesh — blended from
// the rendered views that see them, by visibility against the depth of the surface itself and by viewing angle.  The colour counterpart of
// k_tsdf_integrate (mesh_tsdf.hip), with the same conventions: the caller's stream and buffers, no allocation, no host synchronisation,
// no float atomics.  The rules are in include/customnerf_hip.h; the NumPy restatement the tests pin them to: tests/view_colors_restatement.py.
//
//   k_view_colors_accumulate : one thread per point, in the caller's order (texels arrive in atlas order, so a wave's points are spatial
//                              neighbours and their 2 x 2 footprints share cache lines).  The point's state (16 bytes) and count are read
//                              once, the launch's views (at most VC_BATCH, passed by value: wave-uniform, so the cameras sit in scalar
//                              registers) are walked in index order with the sums in registers, and state and count are written once.  A
//                              point's sums run in view order whatever the cut into launches.  The views are taken VC_UNROLL at a time in
//                              three steps, so that the loads of several views are in flight together: the footprint depths of all of
//                              them, then colour and pixel weight of those that passed the depth test (the others read neither), then the
//                              sums in view order.  The two pixels of a footprint row are one access (8 bytes of depth or weight, 24 of
//                              colour).  What was measured, and what bounds it: profiles/mesh_view_colors.md
//   k_view_colors_resolve    : a thread per point, at most 1024 workgroups striding over them: acc / weight, else the fallback row, else the
//                              fill colour; the points seen by 0, 1 and >= 2 views are counted by ballot, one integer add per workgroup
//                              and class
//
// The camera is the rasteriser's (mesh_camera.h), so a point is compared with the depth that mesh.rasterize wrote for the pixels round it.
#include "mesh_camera.h"

#define VC_BATCH 16
#define VC_UNROLL 4                                              // divides VC_BATCH

namespace {

struct VcViews {
    MeshCam cam[VC_BATCH];
    uint32_t n;                                                  // views of this launch
};

// Steps 1-2 and the view-only parts of 3-4 of the header's rule: the footprint's first pixel (ok: the point lies in front of the camera and
// its whole 2 x 2 footprint in the image; pix = 0 otherwise), the bilinear fractions, the distance r to compare depths with, the cosine
__device__ __forceinline__ bool vc_footprint(const MeshCam &cam, const float p[3], const float n[3], uint32_t H, uint32_t W, int depth_kind,
                                             uint32_t &pix, float &ax, float &ay, float &r, float &cosv) {
    const float d0 = p[0] - cam.m[0][3], d1 = p[1] - cam.m[1][3], d2 = p[2] - cam.m[2][3];
    float z, X, Y;
    mesh_cam_project(cam, d0, d1, d2, z, X, Y);
    bool ok = z >= cam.near;                                     // false behind the camera, nearer than near, or for a NaN
    const float u = X - 0.5f, v = Y - 0.5f, xf = floorf(u), yf = floorf(v);
    ax = u - xf;
    ay = v - yf;
    ok = ok && xf >= 0.0f && xf <= (float)(W - 2) && yf >= 0.0f && yf <= (float)(H - 2);     // W, H >= 2; non-finite values fail
    const uint32_t ix = ok ? (uint32_t)(int)xf : 0u, iy = ok ? (uint32_t)(int)yf : 0u;
    ok = ok && ix + 1 < W && iy + 1 < H;                         // (float)(W - 2) rounded up: only for W > 2^24
    pix = ok ? iy * W + ix : 0u;                                 // H W < 2^31
    const float len = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    r = depth_kind == 0 ? z : len;
    cosv = -((n[0] * d0 + n[1] * d1) + n[2] * d2) / len;
    return ok;
}

// Two pixels of a row side by side, as one access: their address is a multiple of 4, not of the access's size
struct __attribute__((packed, aligned(4))) VcPair {
    float a, b;
};
struct __attribute__((packed, aligned(4))) VcRgbPair {
    float a[3], b[3];
};

// step 3 for one footprint depth: NaN, 0, negative and +inf say "not this surface"
__device__ __forceinline__ bool vc_depth_ok(float D, float r, float tol) { return D > 0.0f && D < INFINITY && fabsf(D - r) <= tol; }

// the bilinear value in the header's fixed order; gx = 1 - ax, gy = 1 - ay
__device__ __forceinline__ float vc_bilerp(float a00, float a10, float a01, float a11, float ax, float ay, float gx, float gy) {
    return (a00 * gx + a10 * ax) * gy + (a01 * gx + a11 * ax) * ay;
}

__global__ __launch_bounds__(MC_BLOCK) void k_view_colors_accumulate(const float *__restrict__ points, const float *__restrict__ normals,
                                                                     uint32_t M, VcViews vs, const float *__restrict__ images,
                                                                     const float *__restrict__ depth, const float *__restrict__ pixel_weight,
                                                                     uint32_t H, uint32_t W, int depth_kind, float depth_tol, float min_cos,
                                                                     int power, float4 *__restrict__ state, uint32_t *__restrict__ seen) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= M) return;
    float p[3], n[3];
    at_load3(points, i, p);
    at_load3(normals, i, n);
    float4 s = state[i];
    uint32_t cnt = seen[i];
    const uint64_t HW = (uint64_t)H * W;
    for (uint32_t v0 = 0; v0 < vs.n; v0 += VC_UNROLL) {          // vs.n is uniform
        bool vis[VC_UNROLL];
        uint64_t base[VC_UNROLL];
        float ax[VC_UNROLL], ay[VC_UNROLL], r[VC_UNROLL], w[VC_UNROLL], D[VC_UNROLL][4];
#pragma unroll
        for (int u = 0; u < VC_UNROLL; ++u) {                    // the footprint depths of VC_UNROLL views
            vis[u] = false;
            base[u] = 0;
            ax[u] = ay[u] = r[u] = w[u] = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) D[u][k] = 0.0f;
            if (v0 + u < vs.n) {                                 // uniform
                uint32_t pix;
                vis[u] = vc_footprint(vs.cam[v0 + u], p, n, H, W, depth_kind, pix, ax[u], ay[u], r[u], w[u]);
                base[u] = (v0 + u) * HW + pix;
                const VcPair d0 = *(const VcPair *)(depth + base[u]), d1 = *(const VcPair *)(depth + base[u] + W);
                D[u][0] = d0.a;                                  // pix = 0 where the point does not project: pixels that exist
                D[u][1] = d0.b;
                D[u][2] = d1.a;
                D[u][3] = d1.b;
            }
        }
        float c[VC_UNROLL][4][3], q[VC_UNROLL][4];
#pragma unroll
        for (int u = 0; u < VC_UNROLL; ++u) {                    // colour and pixel weight only where the depth test passed
            const float cosv = w[u];
#pragma unroll
            for (int k = 0; k < 4; ++k) vis[u] = vis[u] && vc_depth_ok(D[u][k], r[u], depth_tol);
            vis[u] = vis[u] && cosv > min_cos;                   // a NaN cosine fails
            for (int k = 1; k < power; ++k) w[u] = w[u] * cosv;  // power is uniform
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[u][k] = 1.0f;
                c[u][k][0] = c[u][k][1] = c[u][k][2] = 0.0f;
            }
            if (vis[u]) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {                    // the footprint's two rows
                    const uint64_t px = base[u] + (j ? W : 0u);
                    const VcRgbPair t = *(const VcRgbPair *)(images + 3 * px);
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        c[u][2 * j][b] = t.a[b];
                        c[u][2 * j + 1][b] = t.b[b];
                    }
                    if (pixel_weight) {
                        const VcPair t2 = *(const VcPair *)(pixel_weight + px);
                        q[u][2 * j] = t2.a;
                        q[u][2 * j + 1] = t2.b;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < VC_UNROLL; ++u) {                    // in view order
            const float gx = 1.0f - ax[u], gy = 1.0f - ay[u];
            float wv = w[u];
            if (pixel_weight) wv = wv * vc_bilerp(q[u][0], q[u][1], q[u][2], q[u][3], ax[u], ay[u], gx, gy);
            if (vis[u] && wv > 0.0f && wv < INFINITY) {
                s.x += wv * vc_bilerp(c[u][0][0], c[u][1][0], c[u][2][0], c[u][3][0], ax[u], ay[u], gx, gy);
                s.y += wv * vc_bilerp(c[u][0][1], c[u][1][1], c[u][2][1], c[u][3][1], ax[u], ay[u], gx, gy);
                s.z += wv * vc_bilerp(c[u][0][2], c[u][1][2], c[u][2][2], c[u][3][2], ax[u], ay[u], gx, gy);
                s.w += wv;
                cnt += 1u;
            }
        }
    }
    state[i] = s;
    seen[i] = cnt;
}

// at most VC_RESOLVE_BLOCKS workgroups walk the points: every workgroup ends in three integer adds to the same three words, and 65 536
// waves adding there took 0.79 ms for 4.2 M points where the rows stream in a twentieth of that (profiles/mesh_view_colors.md)
#define VC_RESOLVE_BLOCKS 1024

__global__ __launch_bounds__(MC_BLOCK) void k_view_colors_resolve(const float4 *__restrict__ state, const uint32_t *__restrict__ seen, uint32_t M,
                                                                  const float *__restrict__ fallback, float f0, float f1, float f2,
                                                                  float *__restrict__ out, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t red[3][MC_WAVES];
    uint32_t tally[3] = {0u, 0u, 0u};                            // of this wave: the same in every lane
    for (uint32_t base = blockIdx.x * MC_BLOCK; base < M; base += gridDim.x * MC_BLOCK) {        // base is uniform; < 2^31 + 2^18
        const uint32_t i = base + threadIdx.x;
        const bool in = i < M;
        uint32_t cnt = 0;
        if (in) {
            const float4 s = state[i];
            cnt = seen[i];
            const uint64_t o = 3 * (uint64_t)i;
            float c[3] = {f0, f1, f2};
            if (s.w > 0.0f) {
                c[0] = s.x / s.w;
                c[1] = s.y / s.w;
                c[2] = s.z / s.w;
            } else if (fallback) {
                c[0] = fallback[o];
                c[1] = fallback[o + 1];
                c[2] = fallback[o + 2];
            }
            out[o] = c[0];
            out[o + 1] = c[1];
            out[o + 2] = c[2];
        }
        const uint32_t cls = cnt < 2u ? cnt : 2u;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) tally[k] += (uint32_t)__popcll(__ballot(in && cls == k));
    }
    if (cn_lane() == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) red[k][threadIdx.x / CN_WAVE] = tally[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (int j = 0; j < MC_WAVES; ++j) t += red[threadIdx.x][j];
        if (t) atomicAdd(counts + threadIdx.x, (unsigned long long)t);   // integer: any order
    }
}

}  // namespace

extern "C" {

int cnerf_view_colors_accumulate(const float *points, const float *normals, uint32_t M, const float *images, const float *depth,
                                 const float *pixel_weight, uint32_t n_views, uint32_t H, uint32_t W, const float *c2w_host, float fx, float fy,
                                 float cx, float cy, int convention, float near, int depth_kind, float depth_tol, float min_cos, int power,
                                 float *state, uint32_t *seen, void *stream) {
    if (!mesh_cam_ok(fx, fy, cx, cy, near, convention) || depth_kind < 0 || depth_kind > 1 || !(depth_tol > 0.0f && depth_tol < INFINITY) ||
        !(min_cos >= 0.0f && min_cos < 1.0f) || power < 1 || power > 8 || n_views > VC_BATCH || M >= (1u << 31) ||
        (uint64_t)H * W >= (1ull << 31))
        return CNERF_EINVAL;
    if (!M || !n_views) return CNERF_OK;
    if (!points || !normals || !images || !depth || !c2w_host || !state || !seen) return CNERF_ENULL;
    if ((uintptr_t)state & 15) return CNERF_EINVAL;              // a state row is one 16-byte access
    if (H < 2 || W < 2) return CNERF_OK;                         // no 2 x 2 footprint: no view sees any point
    VcViews vs;
    vs.n = n_views;
    for (uint32_t v = 0; v < VC_BATCH; ++v)                       // the slots past vs.n repeat the last view and are never read
        vs.cam[v] = mesh_cam(c2w_host + 12 * (uint64_t)(v < vs.n ? v : vs.n - 1), fx, fy, cx, cy, near, convention);
    hipLaunchKernelGGL(k_view_colors_accumulate, mesh_grid(M), dim3(MC_BLOCK), 0, CN_STREAM(stream), points, normals, M, vs, images, depth,
                       pixel_weight, H, W, depth_kind, depth_tol, min_cos, power, (float4 *)state, seen);
    return cn_launch_status();
}

int cnerf_view_colors_resolve(const float *state, const uint32_t *seen, uint32_t M, const float *fallback, const float *fill_host, float *out,
                              uint64_t *counts, void *stream) {
    if (M >= (1u << 31)) return CNERF_EINVAL;
    if (!M) return CNERF_OK;
    if (!state || !seen || !fill_host || !out || !counts) return CNERF_ENULL;
    if ((uintptr_t)state & 15) return CNERF_EINVAL;
    const uint32_t blocks = cn_div_up(M, MC_BLOCK);
    hipLaunchKernelGGL(k_view_colors_resolve, dim3(blocks < VC_RESOLVE_BLOCKS ? blocks : VC_RESOLVE_BLOCKS), dim3(MC_BLOCK), 0, CN_STREAM(stream), (const float4 *)state, seen, M, fallback,
                       fill_host[0], fill_host[1], fill_host[2], out, (unsigned long long *)counts);
    return cn_launch_status();
}

}  // extern "C"
