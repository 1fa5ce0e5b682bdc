// The arithmetic and the bookkeeping that the two marching-cubes passes share (mesh.hip: a dense volume; mesh_sparse.hip: a list of 8^3
// bricks), in one definition each, so that the two give the same bits: the inside test, the crossing parameter t with its NaN rule, the
// vertex position, the gradient (central inside, one-sided on the LATTICE's faces), the normal, the owner of a table edge, the workspace
// regions of N points and the overflow rule of the two totals.  How a value at an offset from a point is fetched is the caller's: the
// helpers take it as a function.
#pragma once
#include "common.h"
#include "mc_tables.h"
#include "mesh_common.h"

namespace {

struct McPtr {
    uint32_t *flag;                                  // header: [0] the overflow flag, [1] (sparse) open bricks exist
    uint8_t *cases, *masks;
    uint32_t *vbase;
    uint2 *sums;
};

// the workspace regions of n points, in order, from a carver that has handed out nothing yet
inline void mc_take(MeshCarve &c, uint64_t n, McPtr &p) {
    p.flag = c.header();
    p.cases = c.take<uint8_t>(n);
    p.masks = c.take<uint8_t>(n);
    p.vbase = c.take<uint32_t>(n);
    p.sums = c.take<uint2>(cn_div_up64(n, MC_BLOCK));
}

struct McGeom {
    float org[3], sp[3];
};

inline McGeom mc_geom(const float *origin_host, const float *spacing_host) {
    McGeom g;
    for (int b = 0; b < 3; ++b) {
        g.org[b] = origin_host[b];
        g.sp[b] = spacing_host[b];
    }
    return g;
}

__device__ __forceinline__ bool mc_in(float v, float level) { return v >= level; }   // NaN: outside

// where the edge (v0 at 0, v1 at 1) meets the level: clamped to [0, 1]; 0.5 when the quotient is NaN
__device__ __forceinline__ float mc_cross_t(float level, float v0, float v1) {
    const float t = (level - v0) / (v1 - v0);
    return t != t ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
}

// the vertex on the edge of axis a that starts at lattice point idx (global indices)
__device__ __forceinline__ void mc_vertex_pos(const McGeom &g, const uint32_t idx[3], int a, float t, float p[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float fi = (float)idx[b];
        p[b] = b == a ? g.org[b] + (fi + t) * g.sp[b] : g.org[b] + fi * g.sp[b];
    }
}

// d(value)/d(axis) at a point with index idx of len along that axis: central difference inside, one-sided at the lattice's faces, divided
// by the spacing.  val(d) = the value d in {-1, 0, +1} steps along the axis from the point; only existing points are asked for.
template <class Val>
__device__ __forceinline__ float mc_grad(Val val, uint32_t idx, uint32_t len, float sp) {
    const bool lo = idx > 0, hi = idx + 1 < len;
    const float vp = hi ? val(1) : val(0);
    const float vm = lo ? val(-1) : val(0);
    const float h = (lo && hi) ? 2.0f : 1.0f;
    return (vp - vm) / (h * sp);
}

// -(g0 + t (g1 - g0)) normalised (left as it is when its length is not positive)
__device__ __forceinline__ void mc_normal(const float g0[3], const float g1[3], float t, float n[3]) {
    float nv[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) nv[b] = -(g0[b] + t * (g1[b] - g0[b]));
    const float l = sqrtf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
    const float s = l > 0.0f ? l : 1.0f;
#pragma unroll
    for (int b = 0; b < 3; ++b) n[b] = nv[b] / s;
}

// table edge e of a cell -> the corner (bit 0 x, bit 1 y, bit 2 z) whose point owns it and the edge's axis
__device__ __forceinline__ void mc_edge_owner(uint32_t e, uint32_t &corner, uint32_t &axis) {
    corner = cn_mc_edge_corner[e];
    axis = cn_mc_edge_axis[e];
}

// vertex id of the owner's edge of that axis: the owner's base + the rank of the axis among its crossing edges
__device__ __forceinline__ int32_t mc_vertex_id(uint32_t owner_base, uint32_t owner_mask, uint32_t axis) {
    return (int32_t)(owner_base + (uint32_t)__popc(owner_mask & ((1u << axis) - 1u)));
}

// the two totals -> counts[0..1], or 0xffffffff both (and flag[0] = 1) when either exceeds INT32_MAX
__device__ __forceinline__ void mc_store_counts(uint64_t cv, uint64_t ct, uint32_t *__restrict__ counts, uint32_t *__restrict__ flag) {
    const bool over = cv > 0x7fffffffull || ct > 0x7fffffffull;
    counts[0] = over ? 0xffffffffu : (uint32_t)cv;
    counts[1] = over ? 0xffffffffu : (uint32_t)ct;
    flag[0] = over ? 1u : 0u;
}

}  // namespace
