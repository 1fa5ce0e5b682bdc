// What the mesh passes share (mesh.hip: marching cubes, mesh_clean.hip: component removal and clustering, mesh_decimate.hip, mesh_smooth.hip,
// mesh_texture.hip and mesh_charts.hip: the texture atlases).
// Host: the 256-byte alignment, the launch grid and the bump carver every pass describes its workspace with, once.  Device: workgroup
// prefix sums and the one-workgroup scan of workgroup totals, the range-checked face load, the vertex -> list offset steps, the per-vertex
// insertion sort and the compacted vertex store, the lock-free union-find, and the texel -> point helpers of the texture passes.
// Every grid these kernels scan is one thread per item, MC_BLOCK threads per workgroup;
// a count pass stores each workgroup's totals (two as uint2, or N as uint32 [N]), mc_scan_totals / mc_scan_totals_n turn them into exclusive
// offsets in place, and an emit pass adds the in-workgroup prefix (ballot + mbcnt, LDS wave totals) to its workgroup's offset.  Order follows
// the thread index: no atomics.
#pragma once
#include "common.h"

#define MC_BLOCK 256
#define MC_WAVES (MC_BLOCK / CN_WAVE)
#define MC_SCAN_BLOCK 1024
#define MC_SCAN_PER_THREAD 4

namespace {

inline uint64_t mesh_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }
inline dim3 mesh_grid(uint64_t n) { return dim3((uint32_t)cn_div_up64(n, MC_BLOCK)); }      // one thread per item
inline int mesh_check_ws(const void *ws, uint64_t ws_bytes, uint64_t total) {
    return (ws_bytes < total || ((uintptr_t)ws & 15)) ? CNERF_EINVAL : CNERF_OK;
}

// A workspace is a 256-byte header of uint32 slots, then regions of 256-byte-aligned size.  Each pass has one function that takes its
// regions in order and returns total(); without a base (the size query) the pointers are null.
struct MeshCarve {
    uint8_t *base;
    uint64_t off;
    explicit MeshCarve(void *ws) : base((uint8_t *)ws), off(0) {}
    template <class T>
    T *take(uint64_t count) {
        T *p = base ? (T *)(base + off) : nullptr;
        off += mesh_align(sizeof(T) * count);
        return p;
    }
    uint32_t *header() { return take<uint32_t>(64); }
    uint64_t total() const { return off; }
};

__device__ __forceinline__ uint32_t mc_rank(uint64_t ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// exclusive prefix of v (< 2^BITS) over the workgroup in thread order; every thread of the block must call it.  `red` = LDS [MC_WAVES]
template <int BITS>
__device__ __forceinline__ uint32_t mc_block_prefix(uint32_t v, uint32_t *red) {
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < BITS; ++k) {
        const uint64_t b = __ballot((v >> k) & 1u);
        pre += mc_rank(b) << k;
        tot += (uint32_t)__popcll(b) << k;
    }
    const uint32_t w = threadIdx.x / CN_WAVE;
    if (cn_lane() == 0) red[w] = tot;
    __syncthreads();
    for (uint32_t j = 0; j < w; ++j) pre += red[j];
    return pre;
}

// exclusive prefix of any v over the workgroup in thread order and its total; every thread of the block must call it.  `red` = LDS [MC_WAVES]
__device__ __forceinline__ uint32_t mc_block_excl(uint32_t v, uint32_t *red, uint32_t &tot) {
    const uint32_t incl = cn_wave_incl_scan(v), w = threadIdx.x / CN_WAVE;
    if (cn_lane() == CN_WAVE - 1) red[w] = incl;
    __syncthreads();
    uint32_t pre = incl - v;
    tot = 0;
    for (uint32_t j = 0; j < MC_WAVES; ++j) {
        if (j < w) pre += red[j];
        tot += red[j];
    }
    return pre;
}

template <int BITS>
__device__ __forceinline__ uint32_t mc_block_total(uint32_t v, uint32_t *red) {
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < BITS; ++k) tot += (uint32_t)__popcll(__ballot((v >> k) & 1u)) << k;
    if (cn_lane() == 0) red[threadIdx.x / CN_WAVE] = tot;
    __syncthreads();
    uint32_t s = 0;
    for (int j = 0; j < MC_WAVES; ++j) s += red[j];
    return s;
}

// Rank of this thread among the threads before it in its workgroup (thread order) that have the same class c < NC (c >= NC: no class, the
// rank is 0), and every class's workgroup total in tot[]; every thread of the block must call it.  `red` = LDS [NC][MC_WAVES]
template <int NC>
__device__ __forceinline__ uint32_t mc_block_class_rank(uint32_t c, uint32_t (*red)[MC_WAVES], uint32_t tot[NC]) {
    const uint32_t w = threadIdx.x / CN_WAVE, lane = cn_lane();
    uint32_t pre = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const uint64_t b = __ballot(c == (uint32_t)k);
        if (c == (uint32_t)k) pre = mc_rank(b);
        if (lane == 0) red[k][w] = (uint32_t)__popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        uint32_t before = 0, t = 0;
        for (uint32_t j = 0; j < MC_WAVES; ++j) {
            if (j < w) before += red[k][j];
            t += red[k][j];
        }
        tot[k] = t;
        if (c == (uint32_t)k) pre += before;
    }
    return pre;
}

// Body of a one-workgroup (MC_SCAN_BLOCK threads) scan of N counters per workgroup: sums[0..nblk)[N] -> exclusive offsets in place,
// component-wise; tot[] = the N totals (exact in 64 bits; every thread gets them).  Every thread of the block must call it.
template <int N>
__device__ __forceinline__ void mc_scan_totals_n(uint32_t *__restrict__ sums, uint32_t nblk, uint64_t tot[N]) {
    __shared__ uint32_t wsum[N][MC_SCAN_BLOCK / CN_WAVE];
    const uint32_t nw = MC_SCAN_BLOCK / CN_WAVE, w = threadIdx.x / CN_WAVE, lane = cn_lane();
#pragma unroll
    for (int q = 0; q < N; ++q) tot[q] = 0;          // carry: totals of the tiles before this one
    for (uint32_t base = 0; base < nblk; base += MC_SCAN_BLOCK * MC_SCAN_PER_THREAD) {
        const uint32_t j0 = base + threadIdx.x * MC_SCAN_PER_THREAD;
        uint32_t e[N][MC_SCAN_PER_THREAD], s[N], inc[N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            s[q] = 0;
#pragma unroll
            for (int k = 0; k < MC_SCAN_PER_THREAD; ++k) {
                e[q][k] = j0 + k < nblk ? sums[(uint64_t)(j0 + k) * N + q] : 0u;
                s[q] += e[q][k];
            }
            inc[q] = cn_wave_incl_scan(s[q]);
            if (lane == CN_WAVE - 1) wsum[q][w] = inc[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < N; ++q) {
            uint32_t o = inc[q] - s[q], tile = 0;
            for (uint32_t j = 0; j < nw; ++j) {
                if (j < w) o += wsum[q][j];
                tile += wsum[q][j];
            }
            uint64_t p = tot[q] + o;
#pragma unroll
            for (int k = 0; k < MC_SCAN_PER_THREAD; ++k) {
                if (j0 + k < nblk) sums[(uint64_t)(j0 + k) * N + q] = (uint32_t)p;
                p += e[q][k];
            }
            tot[q] += tile;
        }
        __syncthreads();                             // wsum is rewritten by the next tile
    }
}

// the two-counter form: sums as uint2, cv / ct = the two totals
__device__ __forceinline__ void mc_scan_totals(uint2 *__restrict__ sums, uint32_t nblk, uint64_t &cv, uint64_t &ct) {
    uint64_t tot[2];
    mc_scan_totals_n<2>(&sums->x, nblk, tot);
    cv = tot[0];
    ct = tot[1];
}

__device__ __forceinline__ uint32_t mesh_fv(const int32_t *fa, uint32_t f, uint32_t q) { return (uint32_t)fa[3 * (uint64_t)f + q]; }

// the three indices of face f; false when one lies outside [0, V)
__device__ __forceinline__ bool mesh_face(const int32_t *__restrict__ faces, uint32_t f, uint32_t V, uint32_t t[3]) {
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        t[q] = mesh_fv(faces, f, q);
        ok &= t[q] < V;                              // a negative int32 is >= 2^31 > V here
    }
    return ok;
}

// Vertex -> list offsets for two counters per vertex (a, b), one thread per vertex; every thread of the block must call them.
// Count pass: this workgroup's two totals, which a one-workgroup mc_scan_totals turns into offsets.
__device__ __forceinline__ void mesh_csr_totals(uint32_t a, uint32_t b, uint2 *__restrict__ sums) {
    __shared__ uint32_t red_a[MC_WAVES], red_b[MC_WAVES];
    uint32_t ta, tb;
    mc_block_excl(a, red_a, ta);
    mc_block_excl(b, red_b, tb);
    if (threadIdx.x == 0) sums[blockIdx.x] = make_uint2(ta, tb);
}

// Offset pass, per counter: this thread's list start = its workgroup's offset + the in-workgroup exclusive prefix.  `red` = LDS [MC_WAVES]
__device__ __forceinline__ uint32_t mesh_csr_start(uint32_t wg_offset, uint32_t v, uint32_t *red) {
    uint32_t tot;
    return wg_offset + mc_block_excl(v, red, tot);
}

// increasing order, in place; the lists are short (a vertex's faces or edge records)
__device__ __forceinline__ void mesh_isort(uint32_t *l, uint32_t n) {
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t x = l[i];
        uint32_t j = i;
        for (; j > 0 && l[j - 1] > x; --j) l[j] = l[j - 1];
        l[j] = x;
    }
}

// input vertex i becomes output vertex k (its slot in the scan of the keep flags): position, normal when both sides have one, old_index
__device__ __forceinline__ void mesh_emit_vertex(const float *__restrict__ pos, const float *__restrict__ normals, uint32_t i, uint32_t k,
                                                 float *__restrict__ verts_out, float *__restrict__ normals_out,
                                                 int32_t *__restrict__ old_index, uint32_t max_verts) {
    if (k >= max_verts) return;
    const uint64_t s = 3 * (uint64_t)i, d = 3 * (uint64_t)k;
#pragma unroll
    for (int q = 0; q < 3; ++q) verts_out[d + q] = pos[s + q];
    if (normals && normals_out) {
#pragma unroll
        for (int q = 0; q < 3; ++q) normals_out[d + q] = normals[s + q];
    }
    if (old_index) old_index[k] = (int32_t)i;
}

// relaxed agent-scope loads and stores of words other workgroups write in the same pass
__device__ __forceinline__ uint32_t ld_rlx(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_rlx(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Lock-free union-find over uint32 nodes, parent[i] = i at first: the smaller root always wins, so every component's root is its
// smallest node whatever the order of the unions (mesh_clean.hip: vertex components; mesh_charts.hip: charts).
// root of x; shortens the walked path (each visited node gets its grandparent: still an ancestor, so any interleaving is safe)
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x) {
    uint32_t cur = ld_rlx(parent + x);
    if (cur == x) return x;
    uint32_t prev = x, next;
    while (cur > (next = ld_rlx(parent + cur))) {
        st_rlx(parent + prev, next);
        prev = cur;
        cur = next;
    }
    return cur;
}

__device__ __forceinline__ void cc_union(uint32_t *parent, uint32_t a, uint32_t b) {
    uint32_t ra = cc_find(parent, a), rb = cc_find(parent, b);
    while (ra != rb) {
        if (ra < rb) {                               // hook rb under ra; a failed CAS returns rb's current parent: climb from there
            const uint32_t old = atomicCAS(parent + rb, rb, ra);
            if (old == rb) break;
            rb = old;
        } else {
            const uint32_t old = atomicCAS(parent + ra, ra, rb);
            if (old == ra) break;
            ra = old;
        }
    }
}

// What the texture passes share (mesh_texture.hip, mesh_charts.hip): a vertex row, the affine interpolation, the view direction, the
// point / direction store and the uint8 rounding.
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

__device__ __forceinline__ void at_put(float *__restrict__ xo, float *__restrict__ dout, uint32_t q, const float x[3], const float d[3]) {
    const uint64_t o = 3 * (uint64_t)q;
    xo[o] = x[0];
    xo[o + 1] = x[1];
    xo[o + 2] = x[2];
    dout[o] = d[0];
    dout[o + 1] = d[1];
    dout[o + 2] = d[2];
}

__device__ __forceinline__ uint8_t at_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }   // NaN -> 0

}  // namespace
