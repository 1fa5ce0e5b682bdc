// Closest-point and ray queries against a triangle mesh through a bounding-volume hierarchy, and a deterministic surface sampler
// (cnerf_mesh_bvh_*, cnerf_mesh_sample_*): what mesh.distance() measures the deviation between two meshes with, and what mesh.ray_cast(),
// mesh.occluded() and mesh.ambient_occlusion() ask, and what mesh.project_to_surface() moves the texels of a decimated mesh onto the
// full-resolution surface with (cnerf_mesh_bvh_project), and the inside test and signed distance of mesh.winding_number(),
// mesh.contains() and mesh.signed_distance() (cnerf_mesh_winding_*, cnerf_mesh_bvh_signed_distance).  Same conventions as the other mesh passes: the
// caller's stream, buffers and workspace, no allocation, no host synchronisation, no float atomics.  The rules (which faces take part, the
// point-triangle rule, the ray-triangle rule, the sampler's enumeration) are in include/customnerf_hip.h; tests/bvh_restatement.py and
// tests/ray_restatement.py restate them bit for bit.
//
// Build
//   k_bvh_bounds  : per face: index and finiteness check (flags), the number of faces that take part, the box of their centroids (integer
//                   maxima of order-preserving codes: any order of arrival gives the same box)
//   k_bvh_keys    : per face: key = (30-bit Morton code of the centroid in that box << 32) | face; a face left out gets Morton 0xffffffff
//   k_bvh_hist / k_bvh_scan / k_bvh_scatter : LSD radix sort, 8 bits per pass, BV_TILE keys per workgroup.  hist: the tile's 256 digit counts;
//                   scan: mc_scan_totals over the digit-major table (digits 0..127 in .x, 128..255 in .y, the .x total carried into .y);
//                   scatter: the stable rank of a key = its digit's offset + the keys of that digit before it in the tile.  Counts and ranks
//                   come from wave ballots (the lanes holding my digit), one writer per (round, wave, digit): no atomics, so every run moves
//                   every key to the same slot.  The keys are made in face order, so they are already sorted by their low word: the four
//                   passes over bits 32..63 complete the order of the whole 64-bit key.
//   k_bvh_leaves  : per sorted slot: the triangle's record (nine coordinates, face index; 48 B), padded with NaN records to whole leaves;
//                   counts out
//   k_bvh_fit     : one launch per level, deepest first: the boxes.  The tree is implicit and balanced over the sorted order: leaves of
//                   BV_LEAF records, NL of them, depth D = ceil(log2 NL); node (d, j) covers leaves [j NL >> d, (j + 1) NL >> d) and sits at
//                   heap index 2^d + j (children 2 i and 2 i + 1).  No pointers, no atomics, no ordering between workgroups.
// Query
//   k_bvh_closest : one thread per query point, a stackless walk: the path is the heap index, a bit per level says whether the sibling is
//                   still to be visited (nearer child first), so the traversal state is two registers — nothing in LDS or scratch.
//                   Conservative under rounding: a leaf box is grown by 2^-18 of its largest |coordinate| and a subtree is skipped only when
//                   its lower bound, shrunk by 2^-16, is strictly above the best d^2; ties are always visited.  Why that is enough: the
//                   computed closest point x can leave the triangle, and for a far query by much more than ulps (the face region
//                   divides by (va + vb) + vc, whose relative error grows like 2^-23 (|p| / edge)^2).  But an error in v or w moves x
//                   inside the triangle's plane (on an edge: along the edge's line), and p - x of the exact answer is perpendicular
//                   to that plane (line), so such an excursion can only lengthen the computed distance.  What can shorten it is the
//                   rounding of x's coordinates — ulps of the coordinates, covered by the grown box — and of the d^2 arithmetic — ulps
//                   of d^2, covered by the shrink; far away d^2 is dominated by |p|^2 and the shrink dwarfs both.  The tests demand
//                   equality with brute force from the surface out to thousands of diagonals.
//   k_bvh_raycast / k_bvh_occluded : one thread per ray, the same stackless walk (nearer box entry first), for the closest hit (t_max shrinks
//                   to the best hit; a subtree is skipped only when it lies strictly beyond it, so ties reach the smallest-face rule) and for
//                   the any-hit bit (the walk ends at the first face accepted).  The ray/triangle rule is the watertight one of Woop,
//                   Benthin and Wald in the header; bv_ray_box must never skip a face that rule accepts.  With u = 2^-24 and, for a node
//                   box [lo, hi] and a ray origin o, M = the largest |lo[a] - o[a]|, |hi[a] - o[a]| (so |p - o| <= M per axis for every
//                   vertex p under the node, whatever the leaf growth):
//                   (1) sideways.  The rule accepts a face only when 0 lies in the triangle of its three sheared points, whose edge
//                   functions have the right sign (a float32 difference of two rounded products cannot take the wrong sign, and a zero is
//                   redone exactly).  A sheared coordinate is (p - o)[kx] - (d[kx] / d[kz]) (p - o)[kz] up to four roundings (the
//                   difference p - o twice, Sx, the product, the difference) of quantities bounded by 2 M: less than 7 u M.  So some point
//                   P of the real triangle lies within 7 u M, along kx and along ky, of the exact line's point with P's kz coordinate:
//                   the exact line meets the node's box grown by 7 u M.  bv_ray_box grows the box by g = 2^-19 M = 32 u M in
//                   origin-relative coordinates (lo - o is a float32 difference of float32 values: its error is u M, not an ulp of the
//                   coordinates) and intersects the three slabs in the forward parameter w = |d[kz]| t, where the slopes are +-Sx, +-Sy
//                   and +-1: one more product and the rounding of 1 / Sx and of Sx against d[kx] / d[kz] move a slab's end by 3 u of
//                   itself, i.e. the box's side by less than 3 u (M + g).  7 + 2 + 3 < 32.  A direction component so small that 1 / Sx
//                   overflows moves the ray sideways by less than 2^-126 M over the box: the axis is treated as having no motion (the
//                   origin's coordinate must lie in the grown slab), and never meets 0 * inf.
//                   (2) along the ray.  The accepted t is (U Az + V Bz + W Cz) / (U + V + W) with U, V, W of one sign: a weighted mean of
//                   the three Az = Sz (p - o)[kz] with non-negative weights, up to 9 u of the largest |Az|.  So t lies in the node's kz
//                   slab widened by 10 u M / |d[kz]|; the slab bv_ray_box compares with [t_min, t_max] is the one grown by g and costs 2 u
//                   more for |Sz| and the product.  Only the kz slab is compared with the range: for a sliver the float32 weights can be
//                   far from the exact barycentrics, so t need not lie where the exact line crosses the other two slabs.
//                   Both hold while no intermediate overflows or underflows; an empty node is skipped by its inverted box, the NaN
//                   records that pad the last leaf by their face index.  tests/test_gpu_mesh_ray.py demands equality with brute force for
//                   origins on box planes, on faces and thousands of diagonals away.
//   k_bvh_project : one thread per query (x, n, reach) against the tree of the SOURCE mesh: the ray along +n that accepts only faces looking
//                   the way n does (cull 2), the ray along -n that accepts only faces looking back at it (cull 1), the nearer of the two
//                   hits, and where both miss the closest point within reach — what a baker projects a low-polygon mesh's texels with.  It
//                   is the two walks above (bv_trace, bv_nearest), not a third: the two rays go through ONE copy of bv_trace in a loop of
//                   two (the direction's sign and the cull are the loop's only variables), so the kernel's code and registers are those
//                   of a ray cast plus a closest-point walk, and nothing lands in scratch.  The second ray's range ends at
//                   min(reach, t of the first): only a strictly nearer backward hit can win, so the narrowing changes no result and only
//                   prunes.  The closest-point walk is entered by the lanes both rays left without a face and by no others (the lanes of
//                   a wave that hit idle meanwhile; on a baker's input, where the low mesh lies within reach of its source, those are the
//                   texels past a rim).  The walks keep a face, its record's slot and its barycentrics; the point, the interpolated
//                   normal (the one place the source's faces and normals are read) and the offset are made once, after the walks.
// Winding number
//   k_bvh_moments_leaf / k_bvh_moments_fit : per node of the same implicit tree a centre, the radius of a ball about it that holds the
//                   node's vertices, the sum of the faces' area vectors and of their areas — two float4 per heap index in a buffer of
//                   their own, built like the boxes: the deepest level from the records, then one launch per level from the children.
//                   The BVH workspace is read only.
//   k_bvh_winding : one thread per query, the generalized winding number: a depth-first walk, left child first, whose whole state is the
//                   heap index and its depth (the next node: up while a right child, then the right sibling).  A node further away
//                   than beta radii adds its dipole (Barill et al. 2018) from the moments alone — the boxes are never read —
//                   otherwise the walk descends, and a leaf adds the solid angles of its records.  The result depends on the tree,
//                   unlike the queries above: the header fixes every operation, tests/winding_restatement.py restates them.
//   k_bvh_signed  : bv_nearest, unchanged, for the distance and the face; then the winding walk for the sign.  The walks run one after
//                   the other and share only the query point.
// Sampler
//   k_sample_count / k_sample_scan / k_sample_emit : k^2 per face -> workgroup totals -> offsets -> one thread per sample (a binary search in
//                   the workgroup's 256 prefix sums finds its face), so the writes are coalesced whatever the mix of face sizes.
#include "mesh_common.h"

#define BV_BAD_INDEX 1u
#define BV_NONFINITE 2u
#define BV_CLAMPED 4u
#define BV_LEAF 4u
#define BV_KPT 4
#define BV_TILE (MC_BLOCK * BV_KPT)
#define BV_NOFACE 0xffffffffu
#define BV_GROW 3.814697265625e-06f                              // 2^-18
#define BV_SHRINK 0.9999847412109375f                            // 1 - 2^-16
#define BV_MAX_K 256.0f
#define BV_RAY_GROW 1.9073486328125e-06f                         // 2^-19

namespace {

enum { H_N = 0, H_FLAGS = 1, H_CARRY = 2, H_BOX = 4, H_TOTAL = 10 };   // uint32 slots of the header (H_BOX: 6, H_TOTAL: 2)

typedef unsigned long long bv_key;

struct BvPtr {
    uint32_t *hdr;
    float4 *tri;                                                 // [BV_LEAF NLmax][3]
    float4 *box;                                                 // [2^(Dmax + 1)][2], heap index, [0] unused
    bv_key *keys[2];                                             // [F] each
    uint2 *sums;                                                 // [128 tiles]
};

inline uint32_t bv_max_leaves(uint64_t F) { return (uint32_t)(F ? cn_div_up64(F, BV_LEAF) : 1); }
inline uint32_t bv_max_depth(uint64_t F) {
    uint32_t d = 0;
    while ((1ull << d) < bv_max_leaves(F)) ++d;
    return d;
}
inline uint32_t bv_tiles(uint64_t F) { return (uint32_t)cn_div_up64(F ? F : 1, BV_TILE); }

// header | records | boxes (what a query reads) | two key buffers | digit table
uint64_t bv_carve(void *ws, uint64_t F, BvPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.tri = c.take<float4>(3ull * BV_LEAF * bv_max_leaves(F));
    p.box = c.take<float4>(2ull << (bv_max_depth(F) + 1));
    p.keys[0] = c.take<bv_key>(F);
    p.keys[1] = c.take<bv_key>(F);
    p.sums = c.take<uint2>(128ull * bv_tiles(F));
    return c.total();
}

__device__ __forceinline__ bool bv_finite(float x) { return fabsf(x) < INFINITY; }

// the nine coordinates of face f; false when it takes no part (flag tells why)
__device__ __forceinline__ bool bv_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t f, uint32_t V, float x[9],
                                        uint32_t &flag) {
    uint32_t t[3];
    if (!mesh_face(faces, f, V, t)) {
        flag = BV_BAD_INDEX;
        return false;
    }
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            x[3 * k + a] = verts[3 * (uint64_t)t[k] + a];
            fin &= bv_finite(x[3 * k + a]);
        }
    flag = fin ? 0u : BV_NONFINITE;
    return fin;
}

__device__ __forceinline__ float bv_centroid(const float x[9], int a) { return ((x[a] + x[3 + a]) + x[6 + a]) / 3.0f; }

// order-preserving code of a float, and back
__device__ __forceinline__ uint32_t bv_ord(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bv_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

__device__ __forceinline__ void bv_shape(uint32_t n, uint32_t &NL, uint32_t &D) {
    NL = (n + BV_LEAF - 1) / BV_LEAF;
    D = NL <= 1 ? 0 : 32 - __clz(NL - 1);
}

// ------------------------------------------------------------------------------------------------ build: keys
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_bounds(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                         BvPtr p) {
    __shared__ uint32_t red[MC_WAVES][6];
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    float x[9];
    uint32_t flag = 0, m[6] = {0, 0, 0, 0, 0, 0};
    const bool ok = f < F && bv_face(verts, faces, f, V, x, flag);
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = bv_ord(bv_centroid(x, a));
            m[a] = ~o;                                           // the minimum as a maximum of the complement: a zeroed header is neutral
            m[3 + a] = o;
        }
    }
    const uint64_t bok = __ballot(ok);
    const uint32_t bfl = (__ballot(flag & BV_BAD_INDEX) ? BV_BAD_INDEX : 0u) | (__ballot(flag & BV_NONFINITE) ? BV_NONFINITE : 0u);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int o = CN_WAVE / 2; o; o >>= 1) m[k] = max(m[k], (uint32_t)__shfl_xor((int)m[k], o));
    const uint32_t w = threadIdx.x / CN_WAVE;
    if (cn_lane() == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[w][k] = m[k];
        if (bok) atomicAdd(p.hdr + H_N, (uint32_t)__popcll(bok));
        if (bfl) atomicOr(p.hdr + H_FLAGS, bfl);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        uint32_t r = 0;
        for (int j = 0; j < MC_WAVES; ++j) r = max(r, red[j][threadIdx.x]);
        if (r) atomicMax(p.hdr + H_BOX + threadIdx.x, r);
    }
}

__device__ __forceinline__ uint32_t bv_spread(uint32_t v) {     // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_keys(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                       BvPtr p) {
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (f >= F) return;
    float x[9];
    uint32_t flag, code = 0xffffffffu;
    if (bv_face(verts, faces, f, V, x, flag)) {
        code = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = bv_unord(~p.hdr[H_BOX + a]), hi = bv_unord(p.hdr[H_BOX + 3 + a]);
            const float t = ((bv_centroid(x, a) - lo) / (hi - lo)) * 1024.0f;
            const uint32_t q = t >= 0.0f ? (uint32_t)fminf(t, 1023.0f) : 0u;      // NaN (a flat box) -> 0
            code |= bv_spread(q) << a;
        }
    }
    p.keys[0][f] = ((bv_key)code << 32) | f;
}

// ------------------------------------------------------------------------------------------------ build: radix sort
// This workgroup's tile: key[k] = element tile + k MC_BLOCK + thread, rank[k] = the keys with its digit before it in its wave's round,
// cnt[k][w][digit] = the keys with that digit in round k of wave w.  Every thread of the block must call it.
__device__ __forceinline__ void bv_digits(const bv_key *__restrict__ keys, uint32_t N, uint32_t shift, bv_key key[BV_KPT], uint32_t digit[BV_KPT],
                                          uint32_t rank[BV_KPT], uint32_t (*cnt)[MC_WAVES][256]) {
    for (uint32_t i = threadIdx.x; i < BV_KPT * MC_WAVES * 256; i += MC_BLOCK) (&cnt[0][0][0])[i] = 0;
    __syncthreads();
    const uint32_t w = threadIdx.x / CN_WAVE;
#pragma unroll
    for (int k = 0; k < BV_KPT; ++k) {
        const uint64_t i = (uint64_t)blockIdx.x * BV_TILE + (uint32_t)k * MC_BLOCK + threadIdx.x;
        const bool valid = i < N;
        key[k] = valid ? keys[i] : 0;
        const uint32_t d = (uint32_t)(key[k] >> shift) & 255u;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bal = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bal : ~bal;
        }
        digit[k] = valid ? d : 256u;
        rank[k] = mc_rank(peers);
        if (valid && rank[k] == 0) cnt[k][w][d] = (uint32_t)__popcll(peers);
    }
    __syncthreads();
}

// digit t of tile b in the digit-major table: digits below 128 in .x, the others in .y
__device__ __forceinline__ uint32_t &bv_slot(uint2 *sums, uint32_t tiles, uint32_t t, uint32_t b) {
    uint2 &e = sums[(uint64_t)(t & 127u) * tiles + b];
    return (t >> 7) ? e.y : e.x;
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_hist(const bv_key *__restrict__ keys, uint32_t N, uint32_t shift, BvPtr p) {
    __shared__ uint32_t cnt[BV_KPT][MC_WAVES][256];
    bv_key key[BV_KPT];
    uint32_t digit[BV_KPT], rank[BV_KPT];
    bv_digits(keys, N, shift, key, digit, rank, cnt);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < BV_KPT; ++k)
#pragma unroll
        for (int w = 0; w < MC_WAVES; ++w) s += cnt[k][w][threadIdx.x];
    bv_slot(p.sums, gridDim.x, threadIdx.x, blockIdx.x) = s;
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_bvh_scan(uint32_t entries, BvPtr p) {
    uint64_t cx, cy;
    mc_scan_totals(p.sums, entries, cx, cy);                     // cx + cy = N < 2^31
    if (threadIdx.x == 0) p.hdr[H_CARRY] = (uint32_t)cx;
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_scatter(const bv_key *__restrict__ keys, bv_key *__restrict__ out, uint32_t N, uint32_t shift,
                                                          BvPtr p) {
    __shared__ uint32_t cnt[BV_KPT][MC_WAVES][256];
    bv_key key[BV_KPT];
    uint32_t digit[BV_KPT], rank[BV_KPT];
    bv_digits(keys, N, shift, key, digit, rank, cnt);
    uint32_t base = bv_slot(p.sums, gridDim.x, threadIdx.x, blockIdx.x) + ((threadIdx.x >> 7) ? p.hdr[H_CARRY] : 0u);
#pragma unroll
    for (int k = 0; k < BV_KPT; ++k)
#pragma unroll
        for (int w = 0; w < MC_WAVES; ++w) {
            const uint32_t c = cnt[k][w][threadIdx.x];
            cnt[k][w][threadIdx.x] = base;
            base += c;
        }
    __syncthreads();
    const uint32_t w = threadIdx.x / CN_WAVE;
#pragma unroll
    for (int k = 0; k < BV_KPT; ++k) {
        if (digit[k] > 255u) continue;
        const uint32_t dst = cnt[k][w][digit[k]] + rank[k];
        if (dst < N) out[dst] = key[k];                          // always: the offsets of N keys end at N
    }
}

// ------------------------------------------------------------------------------------------------ build: records and boxes
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_leaves(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                         BvPtr p, uint32_t *__restrict__ counts) {
    const uint32_t i = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = p.hdr[H_N];
    if (i == 0) {
        counts[0] = n;
        counts[1] = p.hdr[H_FLAGS];
    }
    if (i >= BV_LEAF * ((n + BV_LEAF - 1) / BV_LEAF)) return;
    float x[9];
    uint32_t f = BV_NOFACE, flag;
    if (i < n) {
        f = (uint32_t)p.keys[0][i];
        if (f >= F || !bv_face(verts, faces, f, V, x, flag)) f = BV_NOFACE;      // never: the first n keys are faces that take part
    }
    if (f == BV_NOFACE)
#pragma unroll
        for (int k = 0; k < 9; ++k) x[k] = __uint_as_float(0x7fc00000u);
    float4 *r = p.tri + 3 * (uint64_t)i;
    r[0] = make_float4(x[0], x[1], x[2], x[3]);
    r[1] = make_float4(x[4], x[5], x[6], x[7]);
    r[2] = make_float4(x[8], __uint_as_float(f), 0.0f, 0.0f);
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_fit(uint32_t d, BvPtr p) {
    const uint32_t j = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = p.hdr[H_N];
    uint32_t NL, D;
    bv_shape(n, NL, D);
    if (!n || d > D || j >= (1u << d)) return;
    const uint64_t idx = ((uint64_t)1 << d) + j;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (d == D) {
        const uint32_t l0 = (uint32_t)(((uint64_t)j * NL) >> D), l1 = (uint32_t)((((uint64_t)j + 1) * NL) >> D);
        for (uint32_t l = l0; l < l1; ++l)                       // none or one
            for (uint32_t t = 0; t < BV_LEAF; ++t) {
                const float4 *r = p.tri + 3 * ((uint64_t)l * BV_LEAF + t);
                const float4 r0 = r[0], r1 = r[1], r2 = r[2];
                if (__float_as_uint(r2.y) == BV_NOFACE) continue;
                const float x[9] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x};
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    lo[k % 3] = fminf(lo[k % 3], x[k]);
                    hi[k % 3] = fmaxf(hi[k % 3], x[k]);
                }
            }
        if (lo[0] <= hi[0]) {
            float s = 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a) s = fmaxf(s, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
            const float g = s * BV_GROW;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] -= g;
                hi[a] += g;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float4 a = p.box[2 * (2 * idx + c)], b = p.box[2 * (2 * idx + c) + 1];
            lo[0] = fminf(lo[0], a.x);
            lo[1] = fminf(lo[1], a.y);
            lo[2] = fminf(lo[2], a.z);
            hi[0] = fmaxf(hi[0], b.x);
            hi[1] = fmaxf(hi[1], b.y);
            hi[2] = fmaxf(hi[2], b.z);
        }
    }
    p.box[2 * idx] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    p.box[2 * idx + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

// ------------------------------------------------------------------------------------------------ query
__device__ __forceinline__ float bv_dot(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// Closest point of triangle (a, b, c) to p (Ericson, Real-Time Collision Detection, 5.1.5), the regions tested in the order A, B, edge AB, C,
// edge AC, edge BC, face: cp, its barycentrics, and d^2 = (dx^2 + dy^2) + dz^2 from the rounded cp.  The order of operations is the header's.
__device__ __forceinline__ float bv_closest(const float p[3], const float a[3], const float b[3], const float c[3], float cp[3], float bary[3]) {
    float ab[3], ac[3], ap[3], bp[3], cq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = b[k] - a[k];
        ac[k] = c[k] - a[k];
        ap[k] = p[k] - a[k];
        bp[k] = p[k] - b[k];
        cq[k] = p[k] - c[k];
    }
    const float d1 = bv_dot(ab, ap), d2 = bv_dot(ac, ap), d3 = bv_dot(ab, bp), d4 = bv_dot(ac, bp), d5 = bv_dot(ab, cq), d6 = bv_dot(ac, cq);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        bary[0] = 1.0f; bary[1] = 0.0f; bary[2] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = a[k];
    } else if (d3 >= 0.0f && d4 <= d3) {
        bary[0] = 0.0f; bary[1] = 1.0f; bary[2] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = b[k];
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        bary[0] = 1.0f - v; bary[1] = v; bary[2] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = a[k] + v * ab[k];
    } else if (d6 >= 0.0f && d5 <= d6) {
        bary[0] = 0.0f; bary[1] = 0.0f; bary[2] = 1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = c[k];
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        bary[0] = 1.0f - w; bary[1] = 0.0f; bary[2] = w;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = a[k] + w * ac[k];
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        bary[0] = 0.0f; bary[1] = 1.0f - w; bary[2] = w;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = b[k] + w * (c[k] - b[k]);
    } else {
        const float denom = 1.0f / ((va + vb) + vc), v = vb * denom, w = vc * denom;
        bary[0] = (1.0f - v) - w; bary[1] = v; bary[2] = w;
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = (a[k] + ab[k] * v) + ac[k] * w;
    }
    const float dx = p[0] - cp[0], dy = p[1] - cp[1], dz = p[2] - cp[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the shrunk lower bound of the squared distance from p to the box of node idx
__device__ __forceinline__ float bv_bound(const float4 *__restrict__ box, uint32_t idx, const float p[3]) {
    const float4 lo = box[2 * (uint64_t)idx], hi = box[2 * (uint64_t)idx + 1];
    const float ex = fmaxf(fmaxf(lo.x - p[0], p[0] - hi.x), 0.0f), ey = fmaxf(fmaxf(lo.y - p[1], p[1] - hi.y), 0.0f);
    const float ez = fmaxf(fmaxf(lo.z - p[2], p[2] - hi.z), 0.0f);
    return ((ex * ex + ey * ey) + ez * ez) * BV_SHRINK;
}

__device__ __forceinline__ uint32_t bv_record(const float4 *__restrict__ tri, uint64_t slot, float a[3], float b[3], float c[3]) {
    const float4 r0 = tri[3 * slot], r1 = tri[3 * slot + 1], r2 = tri[3 * slot + 2];
    a[0] = r0.x; a[1] = r0.y; a[2] = r0.z;
    b[0] = r0.w; b[1] = r1.x; b[2] = r1.y;
    c[0] = r1.z; c[1] = r1.w; c[2] = r2.x;
    return __float_as_uint(r2.y);
}

__device__ __forceinline__ void bv_add_stats(unsigned long long *__restrict__ stats, uint32_t visits, uint32_t tests) {
    const uint32_t sv = cn_wave_sum(visits), st = cn_wave_sum(tests);                     // one pair of adds per wave
    if (cn_lane() == 0 && (sv | st)) {
        atomicAdd(stats, (unsigned long long)sv);
        atomicAdd(stats + 1, (unsigned long long)st);
    }
}

// The walk of k_bvh_closest for the point p (finite, of a tree with n > 0 faces): the smallest d2 (best), the smallest face attaining it
// (bestf, BV_NOFACE: none) and its record (bests).
__device__ __forceinline__ void bv_nearest(const BvPtr &ws, uint32_t n, const float p[3], float &best, uint32_t &bestf, uint32_t &bests,
                                           uint32_t &visits, uint32_t &tests) {
    uint32_t NL, D;
    bv_shape(n, NL, D);
    uint32_t node = 1, depth = 0, pending = 0;                   // pending bit i: the sibling of the path's node i levels up is still to come
    ++visits;
    // until the first triangle is tested best is +inf, and the bound of an empty node (+inf) is not strictly above it: such a node is
    // entered and counted in `visits`; its leaf range is empty, so nothing else changes
    bool go = !(bv_bound(ws.box, 1, p) > best);
    while (go) {
        bool descend = false;
        if (depth == D) {
            const uint32_t j = node - (1u << D);
            const uint32_t l0 = (uint32_t)(((uint64_t)j * NL) >> D), l1 = (uint32_t)((((uint64_t)j + 1) * NL) >> D);
            if (l0 < l1) {
#pragma unroll
                for (uint32_t t = 0; t < BV_LEAF; ++t) {
                    float a[3], b[3], c[3], cp[3], br[3];
                    const uint64_t slot = (uint64_t)l0 * BV_LEAF + t;
                    const uint32_t f = bv_record(ws.tri, slot, a, b, c);
                    if (f == BV_NOFACE) continue;
                    ++tests;
                    const float d2 = bv_closest(p, a, b, c, cp, br);
                    if (d2 < best || (d2 == best && f < bestf)) {       // false for a NaN
                        best = d2;
                        bestf = f;
                        bests = (uint32_t)slot;
                    }
                }
            }
        } else {
            visits += 2;
            const float b0 = bv_bound(ws.box, 2 * node, p), b1 = bv_bound(ws.box, 2 * node + 1, p);
            const bool ok0 = !(b0 > best), ok1 = !(b1 > best);
            if (ok0 || ok1) {
                const uint32_t first = (ok0 && ok1) ? (b1 < b0 ? 1u : 0u) : (ok1 ? 1u : 0u);
                pending = (pending << 1) | ((ok0 && ok1) ? 1u : 0u);
                node = 2 * node + first;
                ++depth;
                descend = true;
            }
        }
        while (!descend) {                                       // back up to the nearest sibling still to come; its box is tested again
            if (!pending) {
                go = false;
                break;
            }
            const uint32_t k = (uint32_t)__ffs((int)pending) - 1;
            node = (node >> k) ^ 1u;
            depth -= k;
            pending = (pending >> k) & ~1u;
            ++visits;
            descend = !(bv_bound(ws.box, node, p) > best);
        }
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_closest(BvPtr ws, uint32_t F, const float *__restrict__ points, uint32_t Q, float *__restrict__ dist2,
                                                          int32_t *__restrict__ face, float *__restrict__ point, float *__restrict__ bary,
                                                          unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);                      // a workspace that was never built must not send the walk out of it
    float p[3] = {0.0f, 0.0f, 0.0f};
    bool live = q < Q && n;
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p[k] = points[3 * (uint64_t)q + k];
            live &= bv_finite(p[k]);
        }
    }
    float best = INFINITY;
    uint32_t bestf = BV_NOFACE, bests = 0, visits = 0, tests = 0;
    if (live) bv_nearest(ws, n, p, best, bestf, bests, visits, tests);
    if (q < Q) {
        const bool hit = bestf != BV_NOFACE;
        dist2[q] = best;
        face[q] = hit ? (int32_t)bestf : -1;
        if (point || bary) {
            float cp[3] = {0.0f, 0.0f, 0.0f}, br[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {
                float a[3], b[3], c[3];
                bv_record(ws.tri, bests, a, b, c);
                bv_closest(p, a, b, c, cp, br);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (point) point[3 * (uint64_t)q + k] = cp[k];
                if (bary) bary[3 * (uint64_t)q + k] = br[k];
            }
        }
    }
    if (stats) bv_add_stats(stats, visits, tests);
}

// ------------------------------------------------------------------------------------------------ rays
__device__ __forceinline__ float bv_pick(const float v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// A ray as the rule of the header sees it (the shear) and as the boxes see it: the forward parameter w = |d[kz]| t, the point at w being
// o + w (+-Sx, +-Sy, +-1) on the axes (kx, ky, kz); rw[a] = w per unit of offset along world axis a (+-1 on kz, +-1 / Sx, +-1 / Sy; not
// finite where the ray does not move along a).  Selects, not indexed arrays: nothing here may land in scratch.
struct BvRay {
    float o[3];
    float sx, sy, sz, asz;                                       // asz = |Sz|: t = w asz
    float rw[3];
    int kx, ky, kz;
};

// false: a degenerate ray (it misses everything)
__device__ __forceinline__ bool bv_ray_setup(const float o[3], const float d[3], BvRay &r) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = o[k];
        ok &= bv_finite(o[k]) && bv_finite(d[k]);
    }
    int kz = 0;
    float m = fabsf(d[0]);
    if (fabsf(d[1]) > m) {
        kz = 1;
        m = fabsf(d[1]);
    }
    if (fabsf(d[2]) > m) {
        kz = 2;
        m = fabsf(d[2]);
    }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = bv_pick(d, kz);
    if (dz < 0.0f) {
        const int s = kx;
        kx = ky;
        ky = s;
    }
    r.kx = kx;
    r.ky = ky;
    r.kz = kz;
    r.sx = bv_pick(d, kx) / dz;
    r.sy = bv_pick(d, ky) / dz;
    r.sz = 1.0f / dz;
    r.asz = fabsf(r.sz);
    const float sg = dz < 0.0f ? -1.0f : 1.0f, rx = sg * (1.0f / r.sx), ry = sg * (1.0f / r.sy);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.rw[a] = a == kz ? sg : (a == kx ? rx : ry);
    return ok && m > 0.0f && bv_finite(r.sx) && bv_finite(r.sy) && bv_finite(r.sz);
}

// The rule of the header for one face: false = a miss whatever the range; true: t and the barycentrics (t may be NaN or infinite; the
// caller's range test decides).
__device__ __forceinline__ bool bv_ray_tri(const BvRay &r, const float a[3], const float b[3], const float c[3], int cull, float &t,
                                           float bary[3]) {
    float A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = a[k] - r.o[k];
        B[k] = b[k] - r.o[k];
        C[k] = c[k] - r.o[k];
    }
    const float Akz = bv_pick(A, r.kz), Bkz = bv_pick(B, r.kz), Ckz = bv_pick(C, r.kz);
    const float Ax = bv_pick(A, r.kx) - r.sx * Akz, Ay = bv_pick(A, r.ky) - r.sy * Akz;
    const float Bx = bv_pick(B, r.kx) - r.sx * Bkz, By = bv_pick(B, r.ky) - r.sy * Bkz;
    const float Cx = bv_pick(C, r.kx) - r.sx * Ckz, Cy = bv_pick(C, r.ky) - r.sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    bool neg, pos;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {                   // on an edge as far as float32 can tell: the products are exact in float64
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx, Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
        const double Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        neg = Ud < 0.0 || Vd < 0.0 || Wd < 0.0;
        pos = Ud > 0.0 || Vd > 0.0 || Wd > 0.0;
        U = (float)Ud;
        V = (float)Vd;
        W = (float)Wd;
    } else {
        neg = U < 0.0f || V < 0.0f || W < 0.0f;
        pos = U > 0.0f || V > 0.0f || W > 0.0f;
    }
    if (neg && pos) return false;
    const float det = (U + V) + W;
    if (det == 0.0f || (cull == 1 && det < 0.0f) || (cull == 2 && det > 0.0f)) return false;
    const float Az = r.sz * Akz, Bz = r.sz * Bkz, Cz = r.sz * Ckz;
    t = ((U * Az + V * Bz) + W * Cz) / det;
    bary[0] = U / det;
    bary[1] = V / det;
    bary[2] = W / det;
    return true;
}

// Can the subtree of node idx hold a face that the rule accepts with t in [tmin, tcur]?  false only when it cannot (the argument is in the
// file header); `enter` = where the ray enters the grown box, in w, for the order of the visit only.
__device__ __forceinline__ bool bv_ray_box(const float4 *__restrict__ box, uint32_t idx, const BvRay &r, float tmin, float tcur, float &enter) {
    const float4 lo = box[2 * (uint64_t)idx], hi = box[2 * (uint64_t)idx + 1];
    enter = INFINITY;
    if (!(lo.x <= hi.x)) return false;                           // a node without leaves
    const float l[3] = {lo.x - r.o[0], lo.y - r.o[1], lo.z - r.o[2]}, h[3] = {hi.x - r.o[0], hi.y - r.o[1], hi.z - r.o[2]};
    float M = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) M = fmaxf(M, fmaxf(fabsf(l[a]), fabsf(h[a])));
    const float g = M * BV_RAY_GROW;
    float en = -INFINITY, ex = INFINITY, zn = 0.0f, zf = 0.0f;
    bool off = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float el = l[a] - g, eh = h[a] + g, rw = r.rw[a];
        if (fabsf(rw) < INFINITY) {
            const float p = el * rw, q = eh * rw, n = fminf(p, q), f = fmaxf(p, q);
            en = fmaxf(en, n);
            ex = fminf(ex, f);
            if (a == r.kz) {
                zn = n;
                zf = f;
            }
        } else {
            off |= el > 0.0f || eh < 0.0f;                       // no motion along a: the origin's coordinate must lie in the slab
        }
    }
    enter = en;
    return !(off || en > ex || zn * r.asz > tcur || zf * r.asz < tmin);
}

// The walk of k_bvh_closest for a ray.  ANY: leave at the first accepted hit (bestf says whether there was one).  bests: the record of
// the face in bestf.
template <bool ANY>
__device__ __forceinline__ void bv_trace(const BvPtr &ws, uint32_t n, const BvRay &ray, float tmin, float tmax, int cull, float &best,
                                         uint32_t &bestf, uint32_t &bests, float bb[3], uint32_t &visits, uint32_t &tests) {
    uint32_t NL, D;
    bv_shape(n, NL, D);
    uint32_t node = 1, depth = 0, pending = 0;
    float tcur = tmax, e0, e1;
    ++visits;
    bool go = bv_ray_box(ws.box, 1, ray, tmin, tcur, e0);
    while (go) {
        bool descend = false;
        if (depth == D) {
            const uint32_t j = node - (1u << D);
            const uint32_t l0 = (uint32_t)(((uint64_t)j * NL) >> D), l1 = (uint32_t)((((uint64_t)j + 1) * NL) >> D);
            if (l0 < l1) {
#pragma unroll
                for (uint32_t i = 0; i < BV_LEAF; ++i) {
                    float a[3], b[3], c[3], br[3], t;
                    const uint64_t slot = (uint64_t)l0 * BV_LEAF + i;
                    const uint32_t f = bv_record(ws.tri, slot, a, b, c);
                    if (f == BV_NOFACE || (ANY && bestf != BV_NOFACE)) continue;
                    ++tests;
                    if (bv_ray_tri(ray, a, b, c, cull, t, br) && tmin <= t && t <= tmax && (t < best || (t == best && f < bestf))) {
                        best = t;
                        bestf = f;
                        bests = (uint32_t)slot;
                        bb[0] = br[0];
                        bb[1] = br[1];
                        bb[2] = br[2];
                    }
                }
                if (ANY && bestf != BV_NOFACE) break;
                tcur = fminf(tmax, best);
            }
        } else {
            visits += 2;
            const bool ok0 = bv_ray_box(ws.box, 2 * node, ray, tmin, tcur, e0), ok1 = bv_ray_box(ws.box, 2 * node + 1, ray, tmin, tcur, e1);
            if (ok0 || ok1) {
                const uint32_t first = (ok0 && ok1) ? (e1 < e0 ? 1u : 0u) : (ok1 ? 1u : 0u);
                pending = (pending << 1) | ((ok0 && ok1) ? 1u : 0u);
                node = 2 * node + first;
                ++depth;
                descend = true;
            }
        }
        while (!descend) {                                       // back up to the nearest sibling still to come; its box is tested again
            if (!pending) {
                go = false;
                break;
            }
            const uint32_t k = (uint32_t)__ffs((int)pending) - 1;
            node = (node >> k) ^ 1u;
            depth -= k;
            pending = (pending >> k) & ~1u;
            ++visits;
            descend = bv_ray_box(ws.box, node, ray, tmin, tcur, e0);
        }
    }
}

// the ray of thread q and its range; false: no walk (q >= Q, no face in the tree, a degenerate ray, an empty range)
__device__ __forceinline__ bool bv_ray_load(const float *__restrict__ origins, const float *__restrict__ dirs, uint32_t q, uint32_t Q, uint32_t n,
                                            float tmin_s, float tmax_s, const float *__restrict__ tmin_a, const float *__restrict__ tmax_a,
                                            BvRay &ray, float &tmin, float &tmax) {
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    tmin = tmin_s;
    tmax = tmax_s;
    if (q < Q) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = origins[3 * (uint64_t)q + k];
            d[k] = dirs[3 * (uint64_t)q + k];
        }
        if (tmin_a) tmin = tmin_a[q];
        if (tmax_a) tmax = tmax_a[q];
    }
    const bool ok = bv_ray_setup(o, d, ray);
    return ok && q < Q && n && !(tmin > tmax);
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_raycast(BvPtr ws, uint32_t F, const float *__restrict__ origins, const float *__restrict__ dirs,
                                                          uint32_t Q, float tmin_s, float tmax_s, const float *__restrict__ tmin_a,
                                                          const float *__restrict__ tmax_a, int cull, float *__restrict__ t_out,
                                                          int32_t *__restrict__ face_out, float *__restrict__ bary_out,
                                                          unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);
    BvRay ray;
    float tmin, tmax, best = INFINITY, bb[3] = {0.0f, 0.0f, 0.0f};
    uint32_t bestf = BV_NOFACE, bests = 0, visits = 0, tests = 0;
    if (bv_ray_load(origins, dirs, q, Q, n, tmin_s, tmax_s, tmin_a, tmax_a, ray, tmin, tmax))
        bv_trace<false>(ws, n, ray, tmin, tmax, cull, best, bestf, bests, bb, visits, tests);
    if (q < Q) {
        if (t_out) t_out[q] = best;
        if (face_out) face_out[q] = bestf != BV_NOFACE ? (int32_t)bestf : -1;
        if (bary_out)
#pragma unroll
            for (int k = 0; k < 3; ++k) bary_out[3 * (uint64_t)q + k] = bb[k];
    }
    if (stats) bv_add_stats(stats, visits, tests);
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_occluded(BvPtr ws, uint32_t F, const float *__restrict__ origins, const float *__restrict__ dirs,
                                                           uint32_t Q, float tmin_s, float tmax_s, const float *__restrict__ tmin_a,
                                                           const float *__restrict__ tmax_a, int cull, uint8_t *__restrict__ occluded,
                                                           unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);
    BvRay ray;
    float tmin, tmax, best = INFINITY, bb[3];
    uint32_t bestf = BV_NOFACE, bests = 0, visits = 0, tests = 0;
    if (bv_ray_load(origins, dirs, q, Q, n, tmin_s, tmax_s, tmin_a, tmax_a, ray, tmin, tmax))
        bv_trace<true>(ws, n, ray, tmin, tmax, cull, best, bestf, bests, bb, visits, tests);
    if (q < Q) occluded[q] = bestf != BV_NOFACE ? 1 : 0;
    if (stats) bv_add_stats(stats, visits, tests);
}

// ------------------------------------------------------------------------------------------------ projection
// x / sqrt((x0 x0 + x1 x1) + x2 x2) when that sum is positive and finite: at_look of mesh_texture.hip without the sign flip
__device__ __forceinline__ bool bv_unit(const float x[3], float u[3]) {
    const float l2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;
    const float l = sqrtf(l2);
    u[0] = x[0] / l;
    u[1] = x[1] / l;
    u[2] = x[2] / l;
    return true;
}

// One thread per query: the ray along +n (cull 2), the ray along -n (cull 1) over [0, min(reach, t of the first)] — one copy of the walk, run
// twice — and, for the threads both rays left without a face, the closest-point walk.  What the walks keep is a face, its record and its
// barycentrics; point and normal are made from the record afterwards.
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_project(BvPtr ws, uint32_t V, uint32_t F, const int32_t *__restrict__ faces,
                                                          const float *__restrict__ normals, const float *__restrict__ xs,
                                                          const float *__restrict__ ns, uint32_t Q, float reach_s, const float *__restrict__ reach_a,
                                                          float *__restrict__ point, float *__restrict__ normal, float *__restrict__ offset,
                                                          int32_t *__restrict__ face, uint8_t *__restrict__ kind,
                                                          unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);
    float x[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f}, reach = reach_s;
    if (q < Q) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = xs[3 * (uint64_t)q + k];
            d[k] = ns[3 * (uint64_t)q + k];
        }
        if (reach_a) reach = reach_a[q];
    }
    bool live = q < Q && n && reach >= 0.0f && (d[0] != 0.0f || d[1] != 0.0f || d[2] != 0.0f);
#pragma unroll
    for (int k = 0; k < 3; ++k) live &= bv_finite(x[k]) && bv_finite(d[k]);
    float t_hit = INFINITY, bh[3] = {0.0f, 0.0f, 0.0f};
    uint32_t f_hit = BV_NOFACE, s_hit = 0, kd = 0, visits = 0, tests = 0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const float dir[3] = {pass ? -d[0] : d[0], pass ? -d[1] : d[1], pass ? -d[2] : d[2]};
        BvRay ray;
        float best = INFINITY, bb[3] = {0.0f, 0.0f, 0.0f};
        uint32_t bestf = BV_NOFACE, bests = 0;
        // t_hit is +inf until a ray has hit: the first walk's range ends at reach, the second's where only a strictly nearer face can be
        if (bv_ray_setup(x, dir, ray) && live)
            bv_trace<false>(ws, n, ray, 0.0f, fminf(reach, t_hit), pass ? 1 : 2, best, bestf, bests, bb, visits, tests);
        if (bestf != BV_NOFACE && (f_hit == BV_NOFACE || best < t_hit)) {          // a tie goes forward
            t_hit = best;
            f_hit = bestf;
            s_hit = bests;
            bh[0] = bb[0];
            bh[1] = bb[1];
            bh[2] = bb[2];
            kd = 1u + (uint32_t)pass;
        }
    }
    const float nn = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    if (live && kd == 0) {
        float best = INFINITY;
        uint32_t bestf = BV_NOFACE, bests = 0;
        bv_nearest(ws, n, x, best, bestf, bests, visits, tests);
        if (bestf != BV_NOFACE && best <= (reach * reach) * nn) {
            kd = 3;
            f_hit = bestf;
            s_hit = bests;
        }
    }
    if (q < Q) {
        float a[3], b[3], c[3], pt[3] = {x[0], x[1], x[2]}, off = 0.0f;
        if (kd) {
            bv_record(ws.tri, s_hit, a, b, c);
            if (kd == 3) {
                bv_closest(x, a, b, c, pt, bh);
                const float r[3] = {pt[0] - x[0], pt[1] - x[1], pt[2] - x[2]};
                off = bv_dot(r, d) / nn;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) pt[k] = (bh[0] * a[k] + bh[1] * b[k]) + bh[2] * c[k];
                off = kd == 2 ? -t_hit : t_hit;
            }
        }
        if (point)
#pragma unroll
            for (int k = 0; k < 3; ++k) point[3 * (uint64_t)q + k] = pt[k];
        if (offset) offset[q] = off;
        if (face) face[q] = kd ? (int32_t)f_hit : -1;
        if (kind) kind[q] = (uint8_t)kd;
        if (normal) {
            float nm[3] = {0.0f, 0.0f, 1.0f};
            bool ok = false;
            if (kd) {
                uint32_t t[3];
                if (normals && f_hit < F && mesh_face(faces, f_hit, V, t)) {
                    float m[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        m[k] = (bh[0] * normals[3 * (uint64_t)t[0] + k] + bh[1] * normals[3 * (uint64_t)t[1] + k]) +
                               bh[2] * normals[3 * (uint64_t)t[2] + k];
                    ok = bv_unit(m, nm);
                }
                if (!ok) {                                       // the face's geometric normal, (b - a) x (c - a)
                    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
                    const float gn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                    ok = bv_unit(gn, nm);
                }
            }
            if (!ok && !bv_unit(d, nm)) {
                nm[0] = 0.0f;
                nm[1] = 0.0f;
                nm[2] = 1.0f;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) normal[3 * (uint64_t)q + k] = nm[k];
        }
    }
    if (stats) bv_add_stats(stats, visits, tests);
}

// ------------------------------------------------------------------------------------------------ winding number
__device__ __forceinline__ void bv_cross(const float u[3], const float v[3], float c[3]) {
    c[0] = u[1] * v[2] - u[2] * v[1];
    c[1] = u[2] * v[0] - u[0] * v[2];
    c[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ float bv_len(const float u[3]) { return sqrtf(bv_dot(u, u)); }

// the leaves [l0, l1) of node j of the deepest level D (none or one)
__device__ __forceinline__ void bv_leaf_range(uint32_t j, uint32_t NL, uint32_t D, uint32_t &l0, uint32_t &l1) {
    l0 = (uint32_t)(((uint64_t)j * NL) >> D);
    l1 = (uint32_t)((((uint64_t)j + 1) * NL) >> D);
}

// The moments of the deepest level's nodes, by the leaf rule of the header.  One thread per node; the records are read twice (the
// sums, then the radius about the centre the sums give).
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_moments_leaf(BvPtr p, uint32_t F, float4 *__restrict__ mom) {
    const uint32_t j = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(p.hdr[H_N], F);
    uint32_t NL, D, l0, l1;
    bv_shape(n, NL, D);
    if (j >= (1u << D)) return;
    bv_leaf_range(j, NL, D, l0, l1);
    float A = 0.0f, N[3] = {0.0f, 0.0f, 0.0f}, S[3] = {0.0f, 0.0f, 0.0f}, M[3] = {0.0f, 0.0f, 0.0f}, a[3], b[3], c[3];
    uint32_t cnt = 0;
    if (l0 < l1)
        for (uint32_t t = 0; t < BV_LEAF; ++t) {
            if (bv_record(p.tri, (uint64_t)l0 * BV_LEAF + t, a, b, c) == BV_NOFACE) continue;
            const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            float x[3];
            bv_cross(e1, e2, x);
            const float Ai = 0.5f * bv_len(x);
            A = A + Ai;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ck = ((a[k] + b[k]) + c[k]) / 3.0f;
                N[k] = N[k] + 0.5f * x[k];
                S[k] = S[k] + Ai * ck;
                M[k] = M[k] + ck;
            }
            ++cnt;
        }
    float pt[3] = {0.0f, 0.0f, 0.0f}, r = -1.0f;
    if (cnt) {
#pragma unroll
        for (int k = 0; k < 3; ++k) pt[k] = A == 0.0f ? M[k] / (float)cnt : S[k] / A;
        r = 0.0f;
        for (uint32_t t = 0; t < BV_LEAF; ++t) {
            if (bv_record(p.tri, (uint64_t)l0 * BV_LEAF + t, a, b, c) == BV_NOFACE) continue;
            const float da[3] = {a[0] - pt[0], a[1] - pt[1], a[2] - pt[2]}, db[3] = {b[0] - pt[0], b[1] - pt[1], b[2] - pt[2]};
            const float dc[3] = {c[0] - pt[0], c[1] - pt[1], c[2] - pt[2]};
            r = fmaxf(fmaxf(r, bv_len(da)), fmaxf(bv_len(db), bv_len(dc)));
        }
    }
    const uint64_t idx = ((uint64_t)1 << D) + j;
    mom[2 * idx] = make_float4(pt[0], pt[1], pt[2], r);
    mom[2 * idx + 1] = make_float4(N[0], N[1], N[2], A);
}

// The moments of level d < D from the two children, by the inner rule of the header.  One launch per level, deepest first.
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_moments_fit(uint32_t d, BvPtr p, uint32_t F, float4 *__restrict__ mom) {
    const uint32_t j = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(p.hdr[H_N], F);
    uint32_t NL, D;
    bv_shape(n, NL, D);
    if (d >= D || j >= (1u << d)) return;
    const uint64_t idx = ((uint64_t)1 << d) + j;
    const float4 l0 = mom[4 * idx], l1 = mom[4 * idx + 1], r0 = mom[4 * idx + 2], r1 = mom[4 * idx + 3];
    float4 o0, o1;
    if (l0.w < 0.0f) {                                           // an empty child: the other one (empty or not) as it is
        o0 = r0;
        o1 = r1;
    } else if (r0.w < 0.0f) {
        o0 = l0;
        o1 = l1;
    } else {
        const float A = l1.w + r1.w;
        const float pl[3] = {l0.x, l0.y, l0.z}, pr[3] = {r0.x, r0.y, r0.z};
        float pt[3], dl[3], dr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pt[k] = A == 0.0f ? 0.5f * (pl[k] + pr[k]) : (l1.w * pl[k] + r1.w * pr[k]) / A;
            dl[k] = pt[k] - pl[k];
            dr[k] = pt[k] - pr[k];
        }
        o0 = make_float4(pt[0], pt[1], pt[2], fmaxf(bv_len(dl) + l0.w, bv_len(dr) + r0.w));
        o1 = make_float4(l1.x + r1.x, l1.y + r1.y, l1.z + r1.z, A);
    }
    mom[2 * idx] = o0;
    mom[2 * idx + 1] = o1;
}

#define BV_FOURPI 12.566370614359172f

// Omega / 4 pi of the triangle (a, b, c) seen from q (Van Oosterom and Strackee 1983), by the rule of the header
__device__ __forceinline__ float bv_solid(const float q[3], const float A[3], const float B[3], const float C[3]) {
    const float a[3] = {A[0] - q[0], A[1] - q[1], A[2] - q[2]}, b[3] = {B[0] - q[0], B[1] - q[1], B[2] - q[2]};
    const float c[3] = {C[0] - q[0], C[1] - q[1], C[2] - q[2]};
    float x[3];
    bv_cross(b, c, x);
    const float num = bv_dot(a, x);
    if (num == 0.0f) return 0.0f;                                // in the triangle's plane as far as float32 can tell
    const float la = bv_len(a), lb = bv_len(b), lc = bv_len(c);
    const float den = (((la * lb) * lc + bv_dot(a, b) * lc) + bv_dot(b, c) * la) + bv_dot(c, a) * lb;
    return (2.0f * atan2f(num, den)) / BV_FOURPI;
}

// The winding number of the tree's faces about q (finite, of a tree with n > 0 faces): a depth-first walk over the implicit tree, left
// child first; the state is the heap index and its depth.  A node far enough for its radius is taken whole as a dipole (Barill et al.
// 2018, the first term of the expansion), read from the moments alone: the boxes are never touched.  Terms add up in the order met.
__device__ __forceinline__ float bv_winding(const BvPtr &ws, const float4 *__restrict__ mom, uint32_t n, const float q[3], float beta2,
                                            uint32_t &accepted, uint32_t &tests) {
    uint32_t NL, D;
    bv_shape(n, NL, D);
    uint32_t node = 1, depth = 0;
    float w = 0.0f;
    for (;;) {
        const float4 m0 = mom[2 * (uint64_t)node];
        bool down = false;
        if (m0.w >= 0.0f) {                                      // not empty
            const float d[3] = {m0.x - q[0], m0.y - q[1], m0.z - q[2]};
            const float d2 = bv_dot(d, d);
            if (d2 > beta2 * (m0.w * m0.w)) {                    // false for beta = inf, whatever the radius (inf * 0 is NaN)
                const float4 m1 = mom[2 * (uint64_t)node + 1];
                const float nn[3] = {m1.x, m1.y, m1.z};
                w = w + bv_dot(nn, d) / (BV_FOURPI * (d2 * sqrtf(d2)));
                ++accepted;
            } else if (depth == D) {
                uint32_t l0, l1;
                bv_leaf_range(node - (1u << D), NL, D, l0, l1);
                if (l0 < l1) {                                   // always: the node is not empty
#pragma unroll
                    for (uint32_t t = 0; t < BV_LEAF; ++t) {
                        float a[3], b[3], c[3];
                        if (bv_record(ws.tri, (uint64_t)l0 * BV_LEAF + t, a, b, c) == BV_NOFACE) continue;
                        ++tests;
                        w = w + bv_solid(q, a, b, c);
                    }
                }
            } else {
                node = 2 * node;
                ++depth;
                down = true;
            }
        }
        if (!down) {                                             // the next node in depth-first order: up while a right child, then right
            while (node & 1u) {
                node >>= 1;
                --depth;
            }
            if (!node) break;                                    // came up from the root
            node += 1;
        }
    }
    return w;
}

// the query point of thread q; false: no walk (q >= Q, no face in the tree, a non-finite point)
__device__ __forceinline__ bool bv_point_load(const float *__restrict__ points, uint32_t q, uint32_t Q, uint32_t n, float p[3]) {
    bool live = q < Q && n;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = q < Q ? points[3 * (uint64_t)q + k] : 0.0f;
        live &= bv_finite(p[k]);
    }
    return live;
}

__global__ __launch_bounds__(MC_BLOCK) void k_bvh_winding(BvPtr ws, uint32_t F, const float4 *__restrict__ mom, const float *__restrict__ points,
                                                          uint32_t Q, float beta, float *__restrict__ winding,
                                                          unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);
    float p[3], w = 0.0f;
    uint32_t accepted = 0, tests = 0;
    if (bv_point_load(points, q, Q, n, p)) w = bv_winding(ws, mom, n, p, beta * beta, accepted, tests);
    if (q < Q) winding[q] = w;
    if (stats) bv_add_stats(stats, accepted, tests);
}

// The signed distance: the closest-point walk for the magnitude and the face, then the winding walk for the sign (negative inside).
// The two walks run one after the other and share nothing but the query point, so the live state is that of the larger one.
__global__ __launch_bounds__(MC_BLOCK) void k_bvh_signed(BvPtr ws, uint32_t F, const float4 *__restrict__ mom, const float *__restrict__ points,
                                                         uint32_t Q, float beta, float *__restrict__ signed_dist, int32_t *__restrict__ face,
                                                         float *__restrict__ winding, unsigned long long *__restrict__ stats) {
    const uint32_t q = blockIdx.x * MC_BLOCK + threadIdx.x;
    const uint32_t n = min(ws.hdr[H_N], F);
    float p[3], best = INFINITY, w = 0.0f;
    uint32_t bestf = BV_NOFACE, bests = 0, visits = 0, ctests = 0, tests = 0, accepted = 0;
    if (bv_point_load(points, q, Q, n, p)) {
        bv_nearest(ws, n, p, best, bestf, bests, visits, ctests);
        w = bv_winding(ws, mom, n, p, beta * beta, accepted, tests);
    }
    if (q < Q) {
        const float dist = sqrtf(best);
        signed_dist[q] = w >= 0.5f ? -dist : dist;
        face[q] = bestf != BV_NOFACE ? (int32_t)bestf : -1;
        if (winding) winding[q] = w;
    }
    if (stats) bv_add_stats(stats, accepted, tests);
}

inline uint64_t bv_moment_bytes(uint64_t F) { return sizeof(float4) * (2ull << (bv_max_depth(F) + 1)); }

// ------------------------------------------------------------------------------------------------ sampler
struct SmpPtr {
    uint32_t *hdr;
    uint2 *sums;                                                 // [F / 256]: x = the workgroup's samples
};

uint64_t smp_carve(void *ws, uint64_t F, SmpPtr &p) {
    MeshCarve c(ws);
    p.hdr = c.header();
    p.sums = c.take<uint2>(cn_div_up64(F ? F : 1, MC_BLOCK));
    return c.total();
}

// area and subdivision order of a face that takes part
__device__ __forceinline__ uint32_t smp_order(const float x[9], float spacing, float &area, bool &clamped) {
    const float e1x = x[3] - x[0], e1y = x[4] - x[1], e1z = x[5] - x[2], e2x = x[6] - x[0], e2y = x[7] - x[1], e2z = x[8] - x[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    area = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
    const float r = ceilf(sqrtf(2.0f * area) / spacing);
    clamped = r > BV_MAX_K;
    return clamped ? (uint32_t)BV_MAX_K : (r >= 1.0f ? (uint32_t)r : 1u);          // NaN -> 1
}

__global__ __launch_bounds__(MC_BLOCK) void k_sample_count(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                           float spacing, SmpPtr p) {
    __shared__ uint32_t red[MC_WAVES];
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    float x[9], area;
    uint32_t flag = 0, cnt = 0;
    if (f < F && bv_face(verts, faces, f, V, x, flag)) {
        bool clamped;
        const uint32_t k = smp_order(x, spacing, area, clamped);
        cnt = k * k;
        if (clamped) flag = BV_CLAMPED;
    }
    const uint32_t bfl = (__ballot(flag & BV_BAD_INDEX) ? BV_BAD_INDEX : 0u) | (__ballot(flag & BV_NONFINITE) ? BV_NONFINITE : 0u) |
                         (__ballot(flag & BV_CLAMPED) ? BV_CLAMPED : 0u);
    if (bfl && cn_lane() == 0) atomicOr(p.hdr + H_FLAGS, bfl);
    uint32_t tot;
    mc_block_excl(cnt, red, tot);                                // <= 256 * 65536
    if (threadIdx.x == 0) p.sums[blockIdx.x] = make_uint2(tot, 0u);
}

__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_sample_scan(uint32_t nblk, SmpPtr p, unsigned long long *__restrict__ counts) {
    uint64_t cx, cy;
    mc_scan_totals(p.sums, nblk, cx, cy);
    if (threadIdx.x == 0) {
        p.hdr[H_TOTAL] = (uint32_t)cx;
        p.hdr[H_TOTAL + 1] = (uint32_t)(cx >> 32);
        counts[0] = cx;
        counts[1] = p.hdr[H_FLAGS];
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_sample_emit(const float *__restrict__ verts, const int32_t *__restrict__ faces, uint32_t V, uint32_t F,
                                                          float spacing, SmpPtr p, float *__restrict__ points, int32_t *__restrict__ face,
                                                          float *__restrict__ bary, float *__restrict__ weight, uint64_t max_samples) {
    __shared__ uint32_t red[MC_WAVES], start[MC_BLOCK], order[MC_BLOCK];
    __shared__ float fx[9][MC_BLOCK], fw[MC_BLOCK];
    if (p.hdr[H_TOTAL + 1]) return;                              // 2^32 samples or more: the 32-bit offsets do not hold them
    const uint32_t f = blockIdx.x * MC_BLOCK + threadIdx.x;
    float x[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, area = 0.0f;
    uint32_t flag, k = 0;
    if (f < F && bv_face(verts, faces, f, V, x, flag)) {
        bool clamped;
        k = smp_order(x, spacing, area, clamped);
    }
    uint32_t tot;
    start[threadIdx.x] = mc_block_excl(k * k, red, tot);
    order[threadIdx.x] = k;
#pragma unroll
    for (int i = 0; i < 9; ++i) fx[i][threadIdx.x] = x[i];
    fw[threadIdx.x] = k ? area / (float)(k * k) : 0.0f;
    __syncthreads();
    const uint64_t base = p.sums[blockIdx.x].x;
    for (uint32_t s = threadIdx.x; s < tot; s += MC_BLOCK) {
        const uint64_t g = base + s;
        if (g >= max_samples) break;
        uint32_t j = 0;                                          // the last face whose start is <= s: the one that holds sample s
#pragma unroll
        for (uint32_t h = MC_BLOCK / 2; h; h >>= 1)
            if (start[j + h] <= s) j += h;
        const uint32_t kk = order[j], m = s - start[j];
        // row i holds 2 (kk - i) - 1 sub-triangles and starts at i (2 kk - i): i = kk - ceil(sqrt(kk^2 - m))
        const uint32_t t = kk * kk - m;
        uint32_t r = (uint32_t)sqrtf((float)t);
        r += r * r < t ? 1u : 0u;
        const uint32_t i = kk - r, rem = m - i * (2 * kk - i), up = rem & 1u, jj = rem >> 1;
        const float den = (float)(3 * kk);
        const float u = (float)(3 * i + 1 + up) / den, v = (float)(3 * jj + 1 + up) / den, b0 = (1.0f - u) - v;
#pragma unroll
        for (int a = 0; a < 3; ++a) points[3 * g + a] = (fx[a][j] + u * (fx[3 + a][j] - fx[a][j])) + v * (fx[6 + a][j] - fx[a][j]);
        bary[3 * g] = b0;
        bary[3 * g + 1] = u;
        bary[3 * g + 2] = v;
        face[g] = (int32_t)(blockIdx.x * MC_BLOCK + j);
        weight[g] = fw[j];
    }
}

bool bv_sizes_ok(uint32_t V, uint32_t F) { return V < (1u << 31) && F < (1u << 31); }

}  // namespace

extern "C" {

int cnerf_mesh_bvh_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F)) return CNERF_EINVAL;
    BvPtr p;
    *bytes_host = bv_carve(nullptr, F, p);
    return CNERF_OK;
}

int cnerf_mesh_bvh_build(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts,
                         void *stream) {
    if (!ws || !counts || (F && (!faces || (V && !verts)))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F)) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, bv_carve(ws, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(p.hdr, 0, 64 * sizeof(uint32_t), st)) return rc;
    if (const int rc = (int)hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), st)) return rc;
    if (!F) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_bounds, mesh_grid(F), dim3(MC_BLOCK), 0, st, verts, faces, V, F, p);
    hipLaunchKernelGGL(k_bvh_keys, mesh_grid(F), dim3(MC_BLOCK), 0, st, verts, faces, V, F, p);
    const uint32_t tiles = bv_tiles(F);
    for (uint32_t pass = 0; pass < 4; ++pass) {                  // keys[0] -> [1] -> [0] -> [1] -> [0]
        const bv_key *src = p.keys[pass & 1];
        const uint32_t shift = 32 + 8 * pass;
        hipLaunchKernelGGL(k_bvh_hist, dim3(tiles), dim3(MC_BLOCK), 0, st, src, F, shift, p);
        hipLaunchKernelGGL(k_bvh_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, 128u * tiles, p);
        hipLaunchKernelGGL(k_bvh_scatter, dim3(tiles), dim3(MC_BLOCK), 0, st, src, p.keys[(pass + 1) & 1], F, shift, p);
    }
    hipLaunchKernelGGL(k_bvh_leaves, mesh_grid((uint64_t)BV_LEAF * bv_max_leaves(F)), dim3(MC_BLOCK), 0, st, verts, faces, V, F, p, counts);
    for (int d = (int)bv_max_depth(F); d >= 0; --d)
        hipLaunchKernelGGL(k_bvh_fit, mesh_grid(1ull << d), dim3(MC_BLOCK), 0, st, (uint32_t)d, p);
    return cn_launch_status();
}

int cnerf_mesh_bvh_closest(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *points, uint32_t Q, float *dist2,
                           int32_t *face, float *point, float *bary, uint64_t *stats, void *stream) {
    if (!ws || (Q && (!points || !dist2 || !face))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31)) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, bv_carve((void *)ws, F, p))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_closest, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, F, points, Q, dist2, face, point, bary,
                       (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_bvh_raycast(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *origins, const float *dirs, uint32_t Q,
                           float t_min, float t_max, const float *t_min_per_ray, const float *t_max_per_ray, int cull, float *t_out,
                           int32_t *face_out, float *bary_out, uint64_t *stats, void *stream) {
    if (!ws || (Q && (!origins || !dirs))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31) || cull < 0 || cull > 2) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, bv_carve((void *)ws, F, p))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_raycast, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, F, origins, dirs, Q, t_min, t_max, t_min_per_ray,
                       t_max_per_ray, cull, t_out, face_out, bary_out, (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_bvh_occluded(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *origins, const float *dirs, uint32_t Q,
                            float t_min, float t_max, const float *t_min_per_ray, const float *t_max_per_ray, int cull, uint8_t *occluded,
                            uint64_t *stats, void *stream) {
    if (!ws || (Q && (!origins || !dirs || !occluded))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31) || cull < 0 || cull > 2) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, bv_carve((void *)ws, F, p))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_occluded, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, F, origins, dirs, Q, t_min, t_max, t_min_per_ray,
                       t_max_per_ray, cull, occluded, (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_bvh_project(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const int32_t *faces, const float *normals,
                           const float *x, const float *n, uint32_t Q, float reach, const float *reach_per_query, float *point,
                           float *normal, float *offset, int32_t *face, uint8_t *kind, uint64_t *stats, void *stream) {
    if (!ws || (Q && (!x || !n || (F && !faces)))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31) || (!reach_per_query && !(reach >= 0.0f))) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, bv_carve((void *)ws, F, p))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_project, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, V, F, faces, normals, x, n, Q, reach,
                       reach_per_query, point, normal, offset, face, kind, (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_winding_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F)) return CNERF_EINVAL;
    *bytes_host = bv_moment_bytes(F);
    return CNERF_OK;
}

int cnerf_mesh_winding_build(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, void *mom, uint64_t mom_bytes, void *stream) {
    if (!bvh_ws || !mom) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F)) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(bvh_ws, bvh_bytes, bv_carve((void *)bvh_ws, F, p))) return rc;
    if (const int rc = mesh_check_ws(mom, mom_bytes, bv_moment_bytes(F))) return rc;
    hipStream_t st = CN_STREAM(stream);
    const int Dmax = (int)bv_max_depth(F);
    hipLaunchKernelGGL(k_bvh_moments_leaf, mesh_grid(1ull << Dmax), dim3(MC_BLOCK), 0, st, p, F, (float4 *)mom);
    for (int d = Dmax - 1; d >= 0; --d)
        hipLaunchKernelGGL(k_bvh_moments_fit, mesh_grid(1ull << d), dim3(MC_BLOCK), 0, st, (uint32_t)d, p, F, (float4 *)mom);
    return cn_launch_status();
}

int cnerf_mesh_winding_query(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, const void *mom, uint64_t mom_bytes,
                             const float *points, uint32_t Q, float beta, float *winding, uint64_t *stats, void *stream) {
    if (!bvh_ws || !mom || (Q && (!points || !winding))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31) || !(beta >= 1.0f)) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(bvh_ws, bvh_bytes, bv_carve((void *)bvh_ws, F, p))) return rc;
    if (const int rc = mesh_check_ws(mom, mom_bytes, bv_moment_bytes(F))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_winding, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, F, (const float4 *)mom, points, Q, beta, winding,
                       (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_bvh_signed_distance(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, const void *mom, uint64_t mom_bytes,
                                   const float *points, uint32_t Q, float beta, float *signed_dist, int32_t *face, float *winding,
                                   uint64_t *stats, void *stream) {
    if (!bvh_ws || !mom || (Q && (!points || !signed_dist || !face))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || Q >= (1u << 31) || !(beta >= 1.0f)) return CNERF_EINVAL;
    BvPtr p;
    if (const int rc = mesh_check_ws(bvh_ws, bvh_bytes, bv_carve((void *)bvh_ws, F, p))) return rc;
    if (const int rc = mesh_check_ws(mom, mom_bytes, bv_moment_bytes(F))) return rc;
    if (!Q) return CNERF_OK;
    hipLaunchKernelGGL(k_bvh_signed, mesh_grid(Q), dim3(MC_BLOCK), 0, CN_STREAM(stream), p, F, (const float4 *)mom, points, Q, beta, signed_dist,
                       face, winding, (unsigned long long *)stats);
    return cn_launch_status();
}

int cnerf_mesh_sample_workspace_bytes(uint32_t F, uint64_t *bytes_host) {
    if (!bytes_host) return CNERF_ENULL;
    if (F >= (1u << 31)) return CNERF_EINVAL;
    SmpPtr p;
    *bytes_host = smp_carve(nullptr, F, p);
    return CNERF_OK;
}

int cnerf_mesh_sample_count(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, float spacing, void *ws, uint64_t ws_bytes,
                            uint64_t *counts, void *stream) {
    if (!ws || !counts || (F && (!faces || (V && !verts)))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || !(spacing > 0.0f) || !(spacing < INFINITY)) return CNERF_EINVAL;
    SmpPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, smp_carve(ws, F, p))) return rc;
    hipStream_t st = CN_STREAM(stream);
    if (const int rc = (int)hipMemsetAsync(p.hdr, 0, 64 * sizeof(uint32_t), st)) return rc;
    if (const int rc = (int)hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), st)) return rc;
    if (!F) return CNERF_OK;
    hipLaunchKernelGGL(k_sample_count, mesh_grid(F), dim3(MC_BLOCK), 0, st, verts, faces, V, F, spacing, p);
    hipLaunchKernelGGL(k_sample_scan, dim3(1), dim3(MC_SCAN_BLOCK), 0, st, (uint32_t)cn_div_up64(F, MC_BLOCK), p, (unsigned long long *)counts);
    return cn_launch_status();
}

int cnerf_mesh_sample_emit(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, float spacing, void *ws, uint64_t ws_bytes,
                           float *points, int32_t *face, float *bary, float *weight, uint64_t max_samples, void *stream) {
    if (!ws || (F && (!faces || (V && !verts))) || (F && max_samples && (!points || !face || !bary || !weight))) return CNERF_ENULL;
    if (!bv_sizes_ok(V, F) || !(spacing > 0.0f) || !(spacing < INFINITY)) return CNERF_EINVAL;
    SmpPtr p;
    if (const int rc = mesh_check_ws(ws, ws_bytes, smp_carve(ws, F, p))) return rc;
    if (!F || !max_samples) return CNERF_OK;
    hipLaunchKernelGGL(k_sample_emit, mesh_grid(F), dim3(MC_BLOCK), 0, CN_STREAM(stream), verts, faces, V, F, spacing, p, points, face, bary, weight,
                       max_samples);
    return cn_launch_status();
}

}  // extern "C"
