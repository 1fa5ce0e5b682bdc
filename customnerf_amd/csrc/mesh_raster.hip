// Rasteriser of a triangle mesh through a pinhole camera (cnerf_mesh_raster_*): a visibility buffer (face, depth, perspective-correct
// barycentrics per pixel) and a shading pass over it.  Same conventions as the other mesh passes: the caller's stream, buffers and workspace,
// no allocation, no host synchronisation, no float atomics — the winner of a pixel is a 64-bit integer minimum, which does not depend on the
// order of arrival, so the output is bit-reproducible.  The rules are in include/customnerf_hip.h; the NumPy restatement the tests pin them
// to: tests/raster_restatement.py.
//
//   k_raster_vertex  : one thread per vertex: its screen position snapped to 1/256 pixel, 1 / depth and whether it may be drawn (16 B)
//   k_raster_faces   : one thread per face: index check, drop, cull, candidate box.  A box of at most RS_SMALL pixels is rasterised by the
//                      thread; a larger one is appended (any order: it cannot change a minimum) to the list of large faces
//   k_raster_tiles   : one workgroup per RS_TILE x RS_TILE pixel tile: scans the list of large faces for boxes that meet its tile (256 per
//                      step, compacted through LDS), then each wave takes one of them and its lanes stride over box ∩ tile.  A face that
//                      fills the view is spread over every tile's workgroup; no lane ever walks a large box alone
//   k_raster_resolve : one thread per pixel: decodes the key, recomputes the winner's barycentrics, writes face / depth / bary
//   k_raster_shade   : one thread per pixel: vertex colours, texture, normals or depth -> RGB8 and the mask
//
// Coverage and the winner are exact (int64 edge functions on the snapped positions); depth is float32 in the header's operation order.
#include "mesh_camera.h"          // the camera and its vertex transform, shared with mesh_tsdf.hip; mesh_common.h

#define RS_SMALL 16
#define RS_TILE 32
#define RS_BAD_INDEX 1u
#define RS_LIMIT 268435456.0f                                  // 2^28: |xi|, |yi| below it keep every edge function inside int64
#define RS_EMPTY (~0ull)

namespace {

struct RasterWs {
    uint32_t *header;                                            // [0]: faces on the large list
    unsigned long long *keys;                                    // [H W]
    int4 *vrec;                                                  // [V]: xi, yi, bits(1 / z), ok
    int4 *boxes;                                                 // [F]: x0, y0, x1, y1 (pixels, inclusive) of a large face
    uint32_t *lfaces;                                            // [F]: its face index
};

uint64_t rs_carve(void *ws, uint64_t V, uint64_t F, uint64_t HW, RasterWs *w) {
    MeshCarve c(ws);
    RasterWs r;
    r.header = c.header();
    r.keys = c.take<unsigned long long>(HW);
    r.vrec = c.take<int4>(V);
    r.boxes = c.take<int4>(F);
    r.lfaces = c.take<uint32_t>(F);
    if (w) *w = r;
    return c.total();
}

__global__ __launch_bounds__(MC_BLOCK) void k_raster_vertex(const float *__restrict__ verts, uint32_t V, MeshCam cam, int4 *__restrict__ vrec) {
    const uint32_t v = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (v >= V) return;
    const uint64_t o = 3 * (uint64_t)v;
    const float d0 = verts[o] - cam.m[0][3], d1 = verts[o + 1] - cam.m[1][3], d2 = verts[o + 2] - cam.m[2][3];
    float z, X, Y;
    mesh_cam_project(cam, d0, d1, d2, z, X, Y);
    const float rx = rintf(X * 256.0f), ry = rintf(Y * 256.0f);
    const bool ok = fabsf(z) < INFINITY && z >= cam.near && fabsf(X) < INFINITY && fabsf(Y) < INFINITY && fabsf(rx) < RS_LIMIT &&
                    fabsf(ry) < RS_LIMIT;                        // every comparison is false on a NaN
    const float q = 1.0f / z;
    vrec[v] = make_int4(ok ? (int)rx : 0, ok ? (int)ry : 0, (int)__float_as_uint(q), ok ? 1 : 0);
}

// One face on the screen, wound so that A > 0: vertex k of the triangle is input corner perm[k].
struct RasterTri {
    int64_t x[3], y[3], A;
    float q[3];
    int perm[3];
    int x0, y0, x1, y1;                                          // candidate pixels, inclusive, clamped to the image; empty when x0 > x1 or y0 > y1
};

// false: the face draws nothing (zero area or culled).  r = the three vertex records in input order
__device__ __forceinline__ bool rs_setup(const int4 r[3], int cull, uint32_t H, uint32_t W, RasterTri &t) {
    const int64_t ax = (int64_t)r[1].x - r[0].x, ay = (int64_t)r[1].y - r[0].y, bx = (int64_t)r[2].x - r[0].x, by = (int64_t)r[2].y - r[0].y;
    const int64_t A = ax * by - ay * bx;
    if (A == 0 || (cull == 1 && A > 0) || (cull == 2 && A < 0)) return false;
    const bool swap = A < 0;
    t.perm[0] = 0;
    t.perm[1] = swap ? 2 : 1;
    t.perm[2] = swap ? 1 : 2;
    t.A = swap ? -A : A;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int4 s = k == 0 ? r[0] : (k == 1 ? (swap ? r[2] : r[1]) : (swap ? r[1] : r[2]));
        t.x[k] = s.x;
        t.y[k] = s.y;
        t.q[k] = __uint_as_float((uint32_t)s.z);
    }
    const int xmin = min(r[0].x, min(r[1].x, r[2].x)), xmax = max(r[0].x, max(r[1].x, r[2].x));
    const int ymin = min(r[0].y, min(r[1].y, r[2].y)), ymax = max(r[0].y, max(r[1].y, r[2].y));
    // ceil((min - 128) / 256) and floor((max - 128) / 256): the arithmetic shift is the floor
    const int64_t px0 = ((int64_t)xmin + 127) >> 8, px1 = ((int64_t)xmax - 128) >> 8, py0 = ((int64_t)ymin + 127) >> 8, py1 = ((int64_t)ymax - 128) >> 8;
    t.x0 = (int)max(px0, (int64_t)0);
    t.y0 = (int)max(py0, (int64_t)0);
    t.x1 = (int)min(px1, (int64_t)W - 1);
    t.y1 = (int)min(py1, (int64_t)H - 1);
    return true;
}

// the three edge functions at the centre of pixel (ix, iy); true when the pixel is covered
__device__ __forceinline__ bool rs_edges(const RasterTri &t, int ix, int iy, int64_t E[3]) {
    const int64_t px = 256 * (int64_t)ix + 128, py = 256 * (int64_t)iy + 128;
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const int64_t dx = t.x[j] - t.x[i], dy = t.y[j] - t.y[i];
        E[k] = dx * (py - t.y[i]) - dy * (px - t.x[i]);
        in &= E[k] > 0 || (E[k] == 0 && (dy < 0 || (dy == 0 && dx > 0)));
    }
    return in;
}

// b_k = (float) E_k / (float) A, bq_k = b_k q_k, depth = 1 / ((bq_0 + bq_1) + bq_2)
__device__ __forceinline__ float rs_depth(const RasterTri &t, const int64_t E[3], float bq[3]) {
    const float Af = (float)t.A;
#pragma unroll
    for (int k = 0; k < 3; ++k) bq[k] = ((float)E[k] / Af) * t.q[k];
    return 1.0f / ((bq[0] + bq[1]) + bq[2]);
}

__device__ __forceinline__ void rs_pixel(const RasterTri &t, uint32_t f, int ix, int iy, uint32_t W, unsigned long long *__restrict__ keys) {
    int64_t E[3];
    if (!rs_edges(t, ix, iy, E)) return;
    float bq[3];
    const float depth = rs_depth(t, E, bq);
    atomicMin(&keys[(uint64_t)iy * W + ix], ((unsigned long long)__float_as_uint(depth) << 32) | f);
}

// the records of face f's vertices; false when an index lies outside [0, V) or a vertex may not be drawn (`bad` tells which)
__device__ __forceinline__ bool rs_load(const int32_t *__restrict__ faces, uint32_t f, uint32_t V, const int4 *__restrict__ vrec, int4 r[3],
                                        bool &bad) {
    uint32_t idx[3];
    bad = !mesh_face(faces, f, V, idx);
    if (bad) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = vrec[idx[k]];
    return (r[0].w & r[1].w & r[2].w) != 0;
}

__global__ __launch_bounds__(MC_BLOCK) void k_raster_faces(const int32_t *__restrict__ faces, uint32_t V, uint32_t F, uint32_t H, uint32_t W,
                                                           int cull, RasterWs ws, uint32_t *__restrict__ counts) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    bool bad = false, drop = false, large = false;
    RasterTri t;
    if (f < F) {
        int4 r[3];
        const bool ok = rs_load(faces, f, V, ws.vrec, r, bad);
        drop = !ok && !bad;
        if (ok && rs_setup(r, cull, H, W, t) && t.x0 <= t.x1 && t.y0 <= t.y1) {
            const uint64_t n = (uint64_t)(t.x1 - t.x0 + 1) * (uint64_t)(t.y1 - t.y0 + 1);
            large = n > RS_SMALL;
            if (!large)
                for (int iy = t.y0; iy <= t.y1; ++iy)
                    for (int ix = t.x0; ix <= t.x1; ++ix) rs_pixel(t, f, ix, iy, W, ws.keys);
        }
    }
    if (bad) atomicOr(&counts[1], RS_BAD_INDEX);
    // one add per wave for the dropped faces and for the list slots
    const uint64_t bd = __ballot(drop), bl = __ballot(large);
    if (drop && mc_rank(bd) == 0) atomicAdd(&counts[0], (uint32_t)__popcll(bd));
    uint32_t base = 0;
    if (large && mc_rank(bl) == 0) base = atomicAdd(&ws.header[0], (uint32_t)__popcll(bl));
    base = __shfl(base, bl ? __ffsll((unsigned long long)bl) - 1 : 0);
    if (large) {
        const uint32_t slot = base + mc_rank(bl);                // < F: a face takes at most one slot
        ws.boxes[slot] = make_int4(t.x0, t.y0, t.x1, t.y1);
        ws.lfaces[slot] = f;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_raster_tiles(const int32_t *__restrict__ faces, uint32_t V, uint32_t H, uint32_t W, int cull,
                                                           uint32_t tiles_x, RasterWs ws) {
    __shared__ uint32_t hit[MC_BLOCK];
    __shared__ uint32_t nhit;
    const uint32_t L = ws.header[0];
    if (!L) return;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int X0 = (int)(tx * RS_TILE), Y0 = (int)(ty * RS_TILE);
    const int X1 = (int)min((uint64_t)X0 + RS_TILE - 1, (uint64_t)W - 1), Y1 = (int)min((uint64_t)Y0 + RS_TILE - 1, (uint64_t)H - 1);
    const uint32_t wave = threadIdx.x / CN_WAVE, lane = cn_lane();
    for (uint32_t s = 0; s < L; s += MC_BLOCK) {
        if (threadIdx.x == 0) nhit = 0;
        __syncthreads();
        const uint32_t e = s + threadIdx.x;
        if (e < L) {
            const int4 b = ws.boxes[e];
            if (b.x <= X1 && b.z >= X0 && b.y <= Y1 && b.w >= Y0) hit[atomicAdd(&nhit, 1u)] = e;   // LDS, integer: any order
        }
        __syncthreads();
        const uint32_t n = nhit;
        for (uint32_t i = wave; i < n; i += MC_WAVES) {
            const uint32_t f = ws.lfaces[hit[i]];
            int4 r[3];
            bool bad;
            RasterTri t;
            if (!rs_load(faces, f, V, ws.vrec, r, bad) || !rs_setup(r, cull, H, W, t)) continue;    // both held when the face was listed
            const int x0 = max(t.x0, X0), x1 = min(t.x1, X1), y0 = max(t.y0, Y0), y1 = min(t.y1, Y1);
            const uint32_t bw = (uint32_t)(x1 - x0 + 1), cnt = bw * (uint32_t)(y1 - y0 + 1);          // <= RS_TILE^2
            for (uint32_t p = lane; p < cnt; p += CN_WAVE) {
                const uint32_t j = p / bw;
                rs_pixel(t, f, x0 + (int)(p - j * bw), y0 + (int)j, W, ws.keys);
            }
        }
        __syncthreads();                                         // hit / nhit are rewritten by the next step
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_raster_resolve(const int32_t *__restrict__ faces, uint32_t V, uint32_t H, uint32_t W, int cull,
                                                             RasterWs ws, const uint32_t *__restrict__ counts, int32_t *__restrict__ face_out,
                                                             float *__restrict__ depth_out, float *__restrict__ bary_out) {
    const uint64_t p = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= (uint64_t)H * W) return;
    const unsigned long long key = ws.keys[p];
    int32_t fo = -1;
    float depth = INFINITY, beta[3] = {0.0f, 0.0f, 0.0f};
    if (key != RS_EMPTY && !(counts[1] & RS_BAD_INDEX)) {
        const uint32_t f = (uint32_t)key, iy = (uint32_t)(p / W), ix = (uint32_t)(p - (uint64_t)iy * W);
        int4 r[3];
        bool bad;
        RasterTri t;
        if (rs_load(faces, f, V, ws.vrec, r, bad) && rs_setup(r, cull, H, W, t)) {
            int64_t E[3];
            float bq[3];
            rs_edges(t, (int)ix, (int)iy, E);
            rs_depth(t, E, bq);
            fo = (int32_t)f;
            depth = __uint_as_float((uint32_t)(key >> 32));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float b = bq[k] * depth;
                if (t.perm[k] == 0) beta[0] = b;
                else if (t.perm[k] == 1) beta[1] = b;
                else beta[2] = b;
            }
        }
    }
    face_out[p] = fo;
    depth_out[p] = depth;
    bary_out[3 * p] = beta[0];
    bary_out[3 * p + 1] = beta[1];
    bary_out[3 * p + 2] = beta[2];
}

struct RasterShade {
    const int32_t *face;
    const float *depth, *bary;
    const int32_t *faces;
    const uint8_t *colors;
    const float *uvs;
    const uint8_t *texture;
    const float *verts, *normals;
    uint32_t HW, V, F, R;
    int mode;
    float d0, d1;
    uchar3 bg;
};

__device__ __forceinline__ uint8_t rs_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }   // NaN -> 0

// x / |x| when |x|^2 is positive and finite
__device__ __forceinline__ bool rs_unit(const float x[3], float n[3]) {
    const float l2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;
    const float l = sqrtf(l2);
#pragma unroll
    for (int q = 0; q < 3; ++q) n[q] = x[q] / l;
    return true;
}

__device__ __forceinline__ const uint8_t *rs_texel(const RasterShade &s, int X, int Y) {
    const int R = (int)s.R;
    return s.texture + 3 * ((uint64_t)min(max(Y, 0), R - 1) * s.R + (uint32_t)min(max(X, 0), R - 1));
}

__global__ __launch_bounds__(MC_BLOCK) void k_raster_shade(RasterShade s, uint8_t *__restrict__ image, uint8_t *__restrict__ mask) {
    const uint64_t p = (uint64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= s.HW) return;
    const int32_t f = s.face[p];
    uchar3 c = s.bg;
    uint8_t m = 0;
    uint32_t idx[3];
    if (f >= 0 && (uint32_t)f < s.F && mesh_face(s.faces, (uint32_t)f, s.V, idx)) {
        m = 255;
        const float b0 = s.bary[3 * p], b1 = s.bary[3 * p + 1], b2 = s.bary[3 * p + 2];
        float x[3];
        if (s.mode == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                x[q] = ((b0 * (float)s.colors[3 * (uint64_t)idx[0] + q] + b1 * (float)s.colors[3 * (uint64_t)idx[1] + q]) +
                        b2 * (float)s.colors[3 * (uint64_t)idx[2] + q]) / 255.0f;
        } else if (s.mode == 1) {
            const float *uv = s.uvs + 6 * (uint64_t)f;
            const float u = (b0 * uv[0] + b1 * uv[2]) + b2 * uv[4], v = (b0 * uv[1] + b1 * uv[3]) + b2 * uv[5];
            const float Rf = (float)s.R, px = u * Rf - 0.5f, py = (1.0f - v) * Rf - 0.5f;
            const float fx0 = floorf(px), fy0 = floorf(py), wx = px - fx0, wy = py - fy0;
            const float lim = 32768.0f;                           // far outside the image either way: the clamp decides
            const int X = (int)fminf(fmaxf(fx0, -lim), lim), Y = (int)fminf(fmaxf(fy0, -lim), lim);   // NaN -> -lim
            const uint8_t *t00 = rs_texel(s, X, Y), *t10 = rs_texel(s, X + 1, Y), *t01 = rs_texel(s, X, Y + 1), *t11 = rs_texel(s, X + 1, Y + 1);
            const float w00 = (1.0f - wx) * (1.0f - wy), w10 = wx * (1.0f - wy), w01 = (1.0f - wx) * wy, w11 = wx * wy;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                x[q] = (((w00 * (float)t00[q] + w10 * (float)t10[q]) + w01 * (float)t01[q]) + w11 * (float)t11[q]) / 255.0f;
        } else if (s.mode == 2) {
            float a[3], n[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q = 0; q < 3; ++q)
                a[q] = (b0 * s.normals[3 * (uint64_t)idx[0] + q] + b1 * s.normals[3 * (uint64_t)idx[1] + q]) + b2 * s.normals[3 * (uint64_t)idx[2] + q];
            if (!rs_unit(a, n)) {                                 // the face's geometric normal, (p1 - p0) x (p2 - p0)
                float e1[3], e2[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    e1[q] = s.verts[3 * (uint64_t)idx[1] + q] - s.verts[3 * (uint64_t)idx[0] + q];
                    e2[q] = s.verts[3 * (uint64_t)idx[2] + q] - s.verts[3 * (uint64_t)idx[0] + q];
                }
                const float g[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                if (!rs_unit(g, n)) n[0] = n[1] = n[2] = 0.0f;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) x[q] = 0.5f + 0.5f * n[q];
        } else {
            x[0] = x[1] = x[2] = (s.depth[p] - s.d0) / (s.d1 - s.d0);
        }
        c = make_uchar3(rs_u8(x[0]), rs_u8(x[1]), rs_u8(x[2]));
    }
    image[3 * p] = c.x;
    image[3 * p + 1] = c.y;
    image[3 * p + 2] = c.z;
    mask[p] = m;
}

// sizes every entry point accepts: V, F < 2^31 and H W < 2^31
bool rs_sizes_ok(uint32_t V, uint32_t F, uint32_t H, uint32_t W) {
    return V < (1u << 31) && F < (1u << 31) && (uint64_t)H * W < (1ull << 31);
}

}  // namespace

extern "C" {

int cnerf_mesh_raster_workspace_bytes(uint32_t V, uint32_t F, uint32_t H, uint32_t W, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (!rs_sizes_ok(V, F, H, W)) return CNERF_EINVAL;
    *bytes_host = rs_carve(nullptr, V, F, (uint64_t)H * W, nullptr);
    return CNERF_OK;
}

int cnerf_mesh_raster_visibility(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, const float *c2w_host, float fx, float fy,
                                 float cx, float cy, uint32_t H, uint32_t W, int convention, float near, int cull, void *ws, uint64_t ws_bytes,
                                 int32_t *face_out, float *depth_out, float *bary_out, uint32_t *counts, void *stream) {
    if (!rs_sizes_ok(V, F, H, W) || !mesh_cam_ok(fx, fy, cx, cy, near, convention) || cull < 0 || cull > 2) return CNERF_EINVAL;
    const uint64_t HW = (uint64_t)H * W;
    if (!c2w_host || !counts || !ws || (F && (!faces || (V && !verts))) || (HW && (!face_out || !depth_out || !bary_out))) return CNERF_ENULL;
    RasterWs w;
    if (const int rc = mesh_check_ws(ws, ws_bytes, rs_carve(ws, V, F, HW, &w))) return rc;
    const MeshCam cam = mesh_cam(c2w_host, fx, fy, cx, cy, near, convention);
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), st)) return rc;
    if (const int rc = (int)hipMemsetAsync(w.header, 0, 64 * sizeof(uint32_t), st)) return rc;
    if (!HW) return CNERF_OK;
    if (const int rc = (int)hipMemsetAsync(w.keys, 0xff, HW * sizeof(unsigned long long), st)) return rc;     // RS_EMPTY
    if (F) {
        if (V) hipLaunchKernelGGL(k_raster_vertex, mesh_grid(V), dim3(MC_BLOCK), 0, st, verts, V, cam, w.vrec);
        hipLaunchKernelGGL(k_raster_faces, mesh_grid(F), dim3(MC_BLOCK), 0, st, faces, V, F, H, W, cull, w, counts);
        const uint32_t tiles_x = cn_div_up(W, RS_TILE), tiles_y = cn_div_up(H, RS_TILE);                       // tiles_x tiles_y < 2^31 / 1024 + H + W
        hipLaunchKernelGGL(k_raster_tiles, dim3(tiles_x * tiles_y), dim3(MC_BLOCK), 0, st, faces, V, H, W, cull, tiles_x, w);
    }
    hipLaunchKernelGGL(k_raster_resolve, mesh_grid(HW), dim3(MC_BLOCK), 0, st, faces, V, H, W, cull, w, counts, face_out, depth_out, bary_out);
    return cn_launch_status();
}

int cnerf_mesh_raster_shade(const int32_t *face, const float *depth, const float *bary, uint32_t H, uint32_t W, const int32_t *faces, uint32_t V,
                            uint32_t F, int mode, const uint8_t *colors, const float *uvs, const uint8_t *texture, uint32_t R,
                            const float *verts, const float *normals, float d0, float d1, const uint8_t *bg_host, uint8_t *image, uint8_t *mask,
                            void *stream) {
    if (!rs_sizes_ok(V, F, H, W) || mode < 0 || mode > 3 || (mode == 1 && (R < 1 || R > 16384))) return CNERF_EINVAL;
    const uint64_t HW = (uint64_t)H * W;
    if (!bg_host) return CNERF_ENULL;
    if (!HW) return CNERF_OK;
    if (!face || !bary || !image || !mask || (F && !faces)) return CNERF_ENULL;
    if (F && ((mode == 0 && !colors) || (mode == 1 && (!uvs || !texture)) || (mode == 2 && (!normals || !verts)) || (mode == 3 && !depth)))
        return CNERF_ENULL;
    RasterShade s;
    s.face = face;
    s.depth = depth;
    s.bary = bary;
    s.faces = faces;
    s.colors = colors;
    s.uvs = uvs;
    s.texture = texture;
    s.verts = verts;
    s.normals = normals;
    s.HW = (uint32_t)HW;
    s.V = V;
    s.F = F;
    s.R = R;
    s.mode = mode;
    s.d0 = d0;
    s.d1 = d1;
    s.bg = make_uchar3(bg_host[0], bg_host[1], bg_host[2]);
    hipLaunchKernelGGL(k_raster_shade, mesh_grid(HW), dim3(MC_BLOCK), 0, CN_STREAM(stream), s, image, mask);
    return cn_launch_status();
}

}  // extern "C"
