// The bake every texture atlas layout shares (mesh_texture.hip: the uniform and the area-proportional layout; mesh_charts.hip: the
// projected one): cell texel t -> its image texel and face -> the surface point and view direction (k_bake_points), the tangent-space code of a
// normal there (k_bake_tspace, for normal maps), the colour byte triple (k_bake_store), and the fill colour on the image texels the store pass does not own (k_bake_fill).  A layout is a locator L,
// a small struct passed by value, with members R and F and
//   typename L::Texel  : what find leaves for the other passes; it has e, the image texel Y * R + X, and f, the owning face or -1
//   find<FACE>(t, tx)  : where cell texel t lies and whose it is; false: the texel is nobody's to write.  Without FACE only the sign of
//                        tx.f is asked for (the store pass: an owned texel takes its colour, another the fill colour)
//   bary(tx, w1, w2, corner) : the texel's barycentric weights in its face and the corner it is the texel of (-1: none); false for a
//                        face without area in the layout, whose point is its vertex 0.  The points and the tspace pass ask
//   stored(e)          : image texel e belongs to the store pass.  The fill pass asks this alone (and R), so its locator may be a smaller
//                        struct; FILL_FLAGS says whether its cells depend on the mesh's indices, i.e. whether a bad index stops the fill
// The extern "C" entry points check what is their layout's own and hand the rest (the range, the pointers, the launch) to bake_launch_*.
#pragma once
#include "mesh_common.h"

#define BK_BLOCK 256

namespace {

// The surface point x and the view direction d at weights (w1, w2) of the face with the (range-checked) vertices v at p0, p1, p2; at a
// corner texel the vertex's own values.  d looks against the interpolated vertex normal, else against the geometric face normal, else
// down (0, 0, -1).  flat: x is vertex 0 itself; the weights still go through the normals' interpolation.
__device__ __forceinline__ void at_surface(const float p0[3], const float p1[3], const float p2[3], const float *__restrict__ normals,
                                           const uint32_t v[3], float w1, float w2, int corner, bool flat, float x[3], float d[3]) {
    if (flat) {
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = p0[k];
    } else {
        at_interp(p0, p1, p2, w1, w2, corner, x);
    }
    bool ok = false;
    if (normals) {
        float n0[3], n1[3], n2[3], nn[3];
        at_load3(normals, v[0], n0);
        at_load3(normals, v[1], n1);
        at_load3(normals, v[2], n2);
        at_interp(n0, n1, n2, w1, w2, corner, nn);
        ok = at_look(nn, d);
    }
    if (!ok) {                                               // the face's geometric normal, (p1 - p0) x (p2 - p0)
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

// one thread per cell texel t in [t0, t0 + count): x and d of its face; point 0 looking down for a texel no face owns
template <class L>
__global__ __launch_bounds__(BK_BLOCK) void k_bake_points(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                          const int32_t *__restrict__ faces, L loc, uint32_t t0, uint32_t count,
                                                          const uint32_t *__restrict__ flags, float *__restrict__ xo, float *__restrict__ dout) {
    const uint32_t q = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (q >= count || flags[0]) return;                      // after a bad index nothing is written
    typename L::Texel tx;
    if (!loc.template find<true>(t0 + q, tx)) return;
    float x[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, -1.0f};
    if (tx.f >= 0) {
        uint32_t v[3];
        if ((uint32_t)tx.f >= loc.F || !mesh_face(faces, (uint32_t)tx.f, V, v)) return;
        float p0[3], p1[3], p2[3], w1, w2;                   // the positions first: the weights' arithmetic (fp64 divisions in the projected
        at_load3(verts, v[0], p0);                           // layout) then runs under these loads, not before them
        at_load3(verts, v[1], p1);
        at_load3(verts, v[2], p2);
        int corner;
        const bool flat = !loc.bary(tx, w1, w2, corner);
        at_surface(p0, p1, p2, normals, v, w1, w2, corner, flat, x, d);
    }
    at_put(xo, dout, q, x, d);
}

// The tangent-space code of the object-space normal m at a texel with surface normal N (unit), the three corners' tangents T0..T2 (xyz and
// the sign w) and the weights of at_surface; float32, one rounding per written operation.  t = T' - N (N . T') normalised, T' the
// interpolated tangent; where |t|^2 is no positive normal number, c - N (N . c) normalised, c the unit axis of the smallest |N_k| (the
// lowest on ties).  w is that of the corner with the largest weight (1 - w1 - w2, w1, w2; the lowest on ties), at a corner texel that
// corner's, on a flat face corner 0's.  B = w (N x t); rgb = 0.5 + 0.5 (m . t, m . B, m . N).  own: the normal is N itself, whose code is
// (0.5, 0.5, 1) exactly.
__device__ __forceinline__ float at_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void at_tspace(const float N[3], const float *__restrict__ tangents, uint32_t f, float w1, float w2, int corner,
                                          bool flat, bool own, const float m[3], float rgb[3]) {
    if (own) {                                               // m is N: nothing to compute
        rgb[0] = 0.5f;
        rgb[1] = 0.5f;
        rgb[2] = 1.0f;
        return;
    }
    const float *T = tangents + 12 * (uint64_t)f;
    const float T0[3] = {T[0], T[1], T[2]}, T1[3] = {T[4], T[5], T[6]}, T2[3] = {T[8], T[9], T[10]};
    float Ti[3], t[3];
    at_interp(T0, T1, T2, w1, w2, corner, Ti);
    const float nt = at_dot(N, Ti);
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = Ti[k] - N[k] * nt;
    float q = at_dot(t, t);
    if (!(q >= __FLT_MIN__ && q < INFINITY)) {
        int a = 0;                                           // selects, not N[a]: an indexed register array would live in scratch
        float na = N[0];
        if (fabsf(N[1]) < fabsf(na)) {
            a = 1;
            na = N[1];
        }
        if (fabsf(N[2]) < fabsf(na)) {
            a = 2;
            na = N[2];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = (k == a ? 1.0f : 0.0f) - N[k] * na;
        q = at_dot(t, t);
    }
    const float l = sqrtf(q);
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t[k] / l;
    int sel = corner;
    if (flat) sel = 0;
    if (sel < 0) {
        const float b0 = (1.0f - w1) - w2;
        sel = 0;
        float best = b0;
        if (w1 > best) {
            sel = 1;
            best = w1;
        }
        if (w2 > best) sel = 2;
    }
    const float w = T[4 * sel + 3];
    const float B[3] = {w * (N[1] * t[2] - N[2] * t[1]), w * (N[2] * t[0] - N[0] * t[2]), w * (N[0] * t[1] - N[1] * t[0])};
    rgb[0] = 0.5f + 0.5f * at_dot(m, t);
    rgb[1] = 0.5f + 0.5f * at_dot(m, B);
    rgb[2] = 0.5f + 0.5f * at_dot(m, N);
}

// one thread per cell texel t in [t0, t0 + count): the tangent-space code of m [count][m_stride] at its face, for k_bake_store; N = -d of
// k_bake_points, bit for bit.  (0.5, 0.5, 1) for a texel no face owns
template <class L>
__global__ __launch_bounds__(BK_BLOCK) void k_bake_tspace(const float *__restrict__ verts, const float *__restrict__ normals, uint32_t V,
                                                          const int32_t *__restrict__ faces, const float *__restrict__ tangents, L loc,
                                                          uint32_t t0, uint32_t count, const float *__restrict__ m, uint32_t m_stride,
                                                          const uint32_t *__restrict__ flags, float *__restrict__ rgb) {
    const uint32_t q = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (q >= count || flags[0]) return;
    typename L::Texel tx;
    if (!loc.template find<true>(t0 + q, tx)) return;
    float c[3] = {0.5f, 0.5f, 1.0f};
    if (tx.f >= 0) {
        uint32_t v[3];
        if ((uint32_t)tx.f >= loc.F || !mesh_face(faces, (uint32_t)tx.f, V, v)) return;
        float p0[3], p1[3], p2[3], w1, w2, x[3], d[3];
        at_load3(verts, v[0], p0);
        at_load3(verts, v[1], p1);
        at_load3(verts, v[2], p2);
        int corner;
        const bool flat = !loc.bary(tx, w1, w2, corner);
        at_surface(p0, p1, p2, normals, v, w1, w2, corner, flat, x, d);
        const float N[3] = {-d[0], -d[1], -d[2]};
        float mq[3] = {0.0f, 0.0f, 0.0f};
        if (m) at_load3(m + (uint64_t)q * m_stride, 0, mq);
        at_tspace(N, tangents, (uint32_t)tx.f, w1, w2, corner, flat, !m, mq, c);
    }
    const uint64_t o = 3 * (uint64_t)q;
    rgb[o] = c[0];
    rgb[o + 1] = c[1];
    rgb[o + 2] = c[2];
}

// one thread per cell texel: round(clamp(rgb, 0, 1) * 255) at its image texel, the fill colour on a texel no face owns
template <class L>
__global__ __launch_bounds__(BK_BLOCK) void k_bake_store(L loc, uint32_t t0, uint32_t count, const float *__restrict__ rgb, uint32_t stride,
                                                         uchar3 fill, const uint32_t *__restrict__ flags, uint8_t *__restrict__ image) {
    const uint32_t q = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (q >= count || flags[0]) return;
    typename L::Texel tx;
    if (!loc.template find<false>(t0 + q, tx)) return;
    uchar3 c = fill;
    if (tx.f >= 0) {
        const uint64_t a = (uint64_t)q * stride;
        c = make_uchar3(at_u8(rgb[a]), at_u8(rgb[a + 1]), at_u8(rgb[a + 2]));
    }
    const uint64_t o = 3 * (uint64_t)tx.e;
    image[o] = c.x;
    image[o + 1] = c.y;
    image[o + 2] = c.z;
}

// one thread per image texel: the fill colour on the texels that are not k_bake_store's.  flags is read under L::FILL_FLAGS only
template <class L>
__global__ __launch_bounds__(BK_BLOCK) void k_bake_fill(L loc, uchar3 fill, const uint32_t *__restrict__ flags, uint8_t *__restrict__ image) {
    const uint32_t e = blockIdx.x * BK_BLOCK + threadIdx.x;
    if (e >= loc.R * loc.R || (L::FILL_FLAGS && flags[0]) || loc.stored(e)) return;
    image[3 * (uint64_t)e] = fill.x;
    image[3 * (uint64_t)e + 1] = fill.y;
    image[3 * (uint64_t)e + 2] = fill.z;
}

// host: the cell texels [t0, t1) of a layout with `total` of them; at most max_points points are written
template <class L>
int bake_launch_points(const L &loc, uint64_t total, const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t t0,
                       uint32_t t1, const uint32_t *flags, float *x, float *d, uint32_t max_points, void *stream) {
    if (t0 > t1 || (uint64_t)t1 > total) return CNERF_EINVAL;
    const uint32_t count = (t1 - t0) < max_points ? t1 - t0 : max_points;
    if (!count) return CNERF_OK;
    if (!flags || !faces || !verts || !x || !d) return CNERF_ENULL;
    hipLaunchKernelGGL(k_bake_points<L>, dim3(cn_div_up(count, BK_BLOCK)), dim3(BK_BLOCK), 0, CN_STREAM(stream), verts, normals, V, faces, loc,
                       t0, count, flags, x, d);
    return cn_launch_status();
}

// host: the tangent-space codes of m for the cell texels [t0, t1); at most max_points rows are read and written
template <class L>
int bake_launch_tspace(const L &loc, uint64_t total, const float *verts, const float *normals, uint32_t V, const int32_t *faces,
                       const float *tangents, uint32_t t0, uint32_t t1, const float *m, uint32_t m_stride, const uint32_t *flags, float *rgb,
                       uint32_t max_points, void *stream) {
    if (t0 > t1 || (uint64_t)t1 > total || (m && m_stride < 3)) return CNERF_EINVAL;
    const uint32_t count = (t1 - t0) < max_points ? t1 - t0 : max_points;
    if (!count) return CNERF_OK;
    if (!flags || !faces || !verts || !tangents || !rgb) return CNERF_ENULL;
    hipLaunchKernelGGL(k_bake_tspace<L>, dim3(cn_div_up(count, BK_BLOCK)), dim3(BK_BLOCK), 0, CN_STREAM(stream), verts, normals, V, faces,
                       tangents, loc, t0, count, m, m_stride, flags, rgb);
    return cn_launch_status();
}

template <class L>
int bake_launch_store(const L &loc, uint64_t total, uint32_t t0, uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host,
                      const uint32_t *flags, uint8_t *image, void *stream) {
    if (t0 > t1 || (uint64_t)t1 > total || rgb_stride < 3) return CNERF_EINVAL;
    if (!fill_host) return CNERF_ENULL;
    if (t1 == t0) return CNERF_OK;
    if (!rgb || !flags || !image) return CNERF_ENULL;
    const uchar3 fill = make_uchar3(fill_host[0], fill_host[1], fill_host[2]);
    hipLaunchKernelGGL(k_bake_store<L>, dim3(cn_div_up(t1 - t0, BK_BLOCK)), dim3(BK_BLOCK), 0, CN_STREAM(stream), loc, t0, t1 - t0, rgb,
                       rgb_stride, fill, flags, image);
    return cn_launch_status();
}

template <class L>
int bake_launch_fill(const L &loc, const uint8_t *fill_host, const uint32_t *flags, uint8_t *image, void *stream) {
    if (!fill_host || !image) return CNERF_ENULL;
    const uchar3 fill = make_uchar3(fill_host[0], fill_host[1], fill_host[2]);
    hipLaunchKernelGGL(k_bake_fill<L>, dim3(cn_div_up(loc.R * loc.R, BK_BLOCK)), dim3(BK_BLOCK), 0, CN_STREAM(stream), loc, fill, flags, image);
    return cn_launch_status();
}

}  // namespace
