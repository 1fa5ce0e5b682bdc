// Texture atlas of a triangle mesh and texture baking (cnerf_mesh_atlas_*): a fixed per-face-pair layout, so that the owner of every texel
// follows from its index (no chart search, no packing state).  Same conventions as the other mesh passes: the caller's stream and buffers,
// no allocation, no host synchronisation, no float atomics (the output is bit-reproducible).  The rules are in include/customnerf_hip.h;
// the NumPy restatement the tests pin them to: tests/atlas_restatement.py.
//
//   k_atlas_uvs    : one thread per face corner: its UV (the centre of a corner texel) and the index check into flags bit 0
//   k_atlas_points : one thread per cell texel t in [t0, t1): its face, the surface point at its (unclamped) barycentrics and the view
//                    direction looking at the surface; the field is evaluated on these between this pass and the next
//   k_atlas_store  : one thread per cell texel: round(clamp(rgb, 0, 1) * 255) at its global position, the fill colour on an un-owned texel
//   k_atlas_fill   : one thread per image texel: the fill colour on every texel outside the first P cells (the others are k_atlas_store's)
//
// Every texel is independent: the passes are bound by their stores (24 B of points and directions per texel, 3 B of image per texel).
#include "common.h"

#define AT_BLOCK 256
#define AT_BAD_INDEX 1u

namespace {

struct AtlasGeom {
    uint32_t F, R, n, s, P;
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
    const float X = (float)(cx * g.s + i), Y = (float)(cy * g.s + j), Rf = (float)g.R;
    uvs[2 * (uint64_t)c] = (X + 0.5f) / Rf;
    uvs[2 * (uint64_t)c + 1] = 1.0f - (Y + 0.5f) / Rf;
}

__device__ __forceinline__ void at_load3(const float *__restrict__ a, uint32_t v, float o[3]) {
    const uint64_t b = 3 * (uint64_t)v;
    o[0] = a[b];
    o[1] = a[b + 1];
    o[2] = a[b + 2];
}

// a0 + w1 (a1 - a0) + w2 (a2 - a0), in this order (the build has -ffp-contract=off); at a corner texel (corner >= 0) the vertex's own value
__device__ __forceinline__ void at_interp(const float a0[3], const float a1[3], const float a2[3], float w1, float w2, int corner, float o[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float v = (a0[q] + w1 * (a1[q] - a0[q])) + w2 * (a2[q] - a0[q]);
        o[q] = corner == 0 ? a0[q] : corner == 1 ? a1[q] : corner == 2 ? a2[q] : v;
    }
}

// -x / |x| when |x|^2 is positive and finite
__device__ __forceinline__ bool at_look(const float x[3], float d[3]) {
    const float l2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;
    const float l = sqrtf(l2);
    d[0] = -(x[0] / l);
    d[1] = -(x[1] / l);
    d[2] = -(x[2] / l);
    return true;
}

__global__ __launch_bounds__(AT_BLOCK) void k_atlas_points(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                           const int32_t *__restrict__ faces, AtlasGeom g, uint32_t t0, uint32_t count,
                                                           const uint32_t *__restrict__ flags, float *__restrict__ xo, float *__restrict__ dout) {
    const uint32_t q = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (q >= count || flags[0]) return;                      // after a bad index nothing is written
    const uint32_t s = g.s, s2 = s * s, t = t0 + q;
    const uint32_t p = t / s2, r = t - p * s2, j = r / s, i = r - j * s;
    const uint32_t b = i + j > s - 1 ? 1u : 0u, f = 2 * p + b;
    float x[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, -1.0f};
    if (f < g.F) {
        const int32_t v0 = faces[3 * (uint64_t)f], v1 = faces[3 * (uint64_t)f + 1], v2 = faces[3 * (uint64_t)f + 2];
        if (v0 < 0 || (uint32_t)v0 >= V || v1 < 0 || (uint32_t)v1 >= V || v2 < 0 || (uint32_t)v2 >= V) return;
        float w1, w2;
        int corner;
        if (!b) {
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
        float p0[3], p1[3], p2[3];
        at_load3(verts, (uint32_t)v0, p0);
        at_load3(verts, (uint32_t)v1, p1);
        at_load3(verts, (uint32_t)v2, p2);
        at_interp(p0, p1, p2, w1, w2, corner, x);
        bool ok = false;
        if (normals) {
            float n0[3], n1[3], n2[3], nn[3];
            at_load3(normals, (uint32_t)v0, n0);
            at_load3(normals, (uint32_t)v1, n1);
            at_load3(normals, (uint32_t)v2, n2);
            at_interp(n0, n1, n2, w1, w2, corner, nn);
            ok = at_look(nn, d);
        }
        if (!ok) {                                           // the face's geometric normal, (p1 - p0) x (p2 - p0)
            const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
            const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
            const float gn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            if (!at_look(gn, d)) {
                d[0] = 0.0f;
                d[1] = 0.0f;
                d[2] = -1.0f;
            }
        }
    }
    const uint64_t o = 3 * (uint64_t)q;
    xo[o] = x[0];
    xo[o + 1] = x[1];
    xo[o + 2] = x[2];
    dout[o] = d[0];
    dout[o + 1] = d[1];
    dout[o + 2] = d[2];
}

__device__ __forceinline__ uint8_t at_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }   // NaN -> 0

__global__ __launch_bounds__(AT_BLOCK) void k_atlas_store(AtlasGeom g, uint32_t t0, uint32_t count, const float *__restrict__ rgb,
                                                          uint32_t stride, uchar3 fill, const uint32_t *__restrict__ flags,
                                                          uint8_t *__restrict__ image) {
    const uint32_t q = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (q >= count || flags[0]) return;
    const uint32_t s = g.s, s2 = s * s, t = t0 + q;
    const uint32_t p = t / s2, r = t - p * s2, j = r / s, i = r - j * s;
    const uint32_t f = 2 * p + (i + j > s - 1 ? 1u : 0u);
    const uint32_t cy = p / g.n, cx = p - cy * g.n;
    const uint64_t o = 3 * ((uint64_t)(cy * s + j) * g.R + cx * s + i);
    uchar3 c = fill;
    if (f < g.F) {
        const uint64_t a = (uint64_t)q * stride;
        c = make_uchar3(at_u8(rgb[a]), at_u8(rgb[a + 1]), at_u8(rgb[a + 2]));
    }
    image[o] = c.x;
    image[o + 1] = c.y;
    image[o + 2] = c.z;
}

__global__ __launch_bounds__(AT_BLOCK) void k_atlas_fill(AtlasGeom g, uchar3 fill, uint8_t *__restrict__ image) {
    const uint32_t e = blockIdx.x * AT_BLOCK + threadIdx.x;
    if (e >= g.R * g.R) return;
    const uint32_t Y = e / g.R, X = e - Y * g.R, cx = X / g.s, cy = Y / g.s;
    if (cx < g.n && cy < g.n && cy * g.n + cx < g.P) return;    // a used cell: k_atlas_store writes it
    image[3 * (uint64_t)e] = fill.x;
    image[3 * (uint64_t)e + 1] = fill.y;
    image[3 * (uint64_t)e + 2] = fill.z;
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
    if (V >= (1u << 31) || t0 > t1 || (uint64_t)t1 > (uint64_t)g.P * g.s * g.s) return CNERF_EINVAL;
    const uint32_t count = (t1 - t0) < max_points ? t1 - t0 : max_points;
    if (!count) return CNERF_OK;
    if (!flags || !faces || !verts || !x || !d) return CNERF_ENULL;
    hipLaunchKernelGGL(k_atlas_points, dim3(cn_div_up(count, AT_BLOCK)), dim3(AT_BLOCK), 0, CN_STREAM(stream), verts, normals, V, faces, g, t0,
                       count, flags, x, d);
    return cn_launch_status();
}

int cnerf_mesh_atlas_store(uint32_t F, uint32_t R, uint32_t t0, uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host,
                           const uint32_t *flags, uint8_t *image, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    if (t0 > t1 || (uint64_t)t1 > (uint64_t)g.P * g.s * g.s || rgb_stride < 3) return CNERF_EINVAL;
    if (!fill_host) return CNERF_ENULL;
    if (t1 == t0) return CNERF_OK;
    if (!rgb || !flags || !image) return CNERF_ENULL;
    const uchar3 fill = make_uchar3(fill_host[0], fill_host[1], fill_host[2]);
    hipLaunchKernelGGL(k_atlas_store, dim3(cn_div_up(t1 - t0, AT_BLOCK)), dim3(AT_BLOCK), 0, CN_STREAM(stream), g, t0, t1 - t0, rgb, rgb_stride,
                       fill, flags, image);
    return cn_launch_status();
}

int cnerf_mesh_atlas_fill(uint32_t F, uint32_t R, const uint8_t *fill_host, uint8_t *image, void *stream) {
    AtlasGeom g;
    if (const int rc = at_layout(F, R, &g)) return rc;
    if (!fill_host || !image) return CNERF_ENULL;
    const uchar3 fill = make_uchar3(fill_host[0], fill_host[1], fill_host[2]);
    hipLaunchKernelGGL(k_atlas_fill, dim3(cn_div_up(R * R, AT_BLOCK)), dim3(AT_BLOCK), 0, CN_STREAM(stream), g, fill, image);
    return cn_launch_status();
}

}  // extern "C"
