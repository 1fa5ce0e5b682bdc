// Workgroup prefix sums and the one-workgroup scan of workgroup totals, shared by the mesh kernels (mesh.hip: marching cubes,
// mesh_clean.hip: component removal and clustering, mesh_decimate.hip and mesh_smooth.hip: vertex lists).  Every grid these kernels scan
// is one thread per item, MC_BLOCK threads per workgroup;
// a count pass stores each workgroup's two totals (uint2), mc_scan_totals turns them into exclusive offsets in place, and an emit pass adds
// the in-workgroup prefix (ballot + mbcnt, LDS wave totals) to its workgroup's offset.  Order follows the thread index: no atomics.
#pragma once
#include "common.h"

#define MC_BLOCK 256
#define MC_WAVES (MC_BLOCK / CN_WAVE)
#define MC_SCAN_BLOCK 1024
#define MC_SCAN_PER_THREAD 4

namespace {

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

// Body of a one-workgroup (MC_SCAN_BLOCK threads) scan: sums[0..nblk) -> exclusive offsets in place, component-wise; cv / ct = the two
// totals (exact in 64 bits; every thread gets them).  Every thread of the block must call it.
__device__ __forceinline__ void mc_scan_totals(uint2 *__restrict__ sums, uint32_t nblk, uint64_t &cv, uint64_t &ct) {
    __shared__ uint32_t wv[MC_SCAN_BLOCK / CN_WAVE], wt[MC_SCAN_BLOCK / CN_WAVE];
    const uint32_t nw = MC_SCAN_BLOCK / CN_WAVE, w = threadIdx.x / CN_WAVE, lane = cn_lane();
    cv = 0;                                          // carry: totals of the tiles before this one
    ct = 0;
    for (uint32_t base = 0; base < nblk; base += MC_SCAN_BLOCK * MC_SCAN_PER_THREAD) {
        const uint32_t j0 = base + threadIdx.x * MC_SCAN_PER_THREAD;
        uint2 e[MC_SCAN_PER_THREAD];
        uint32_t sv = 0, st = 0;
#pragma unroll
        for (int k = 0; k < MC_SCAN_PER_THREAD; ++k) {
            e[k] = j0 + k < nblk ? sums[j0 + k] : make_uint2(0, 0);
            sv += e[k].x;
            st += e[k].y;
        }
        const uint32_t iv = cn_wave_incl_scan(sv), it = cn_wave_incl_scan(st);
        if (lane == CN_WAVE - 1) { wv[w] = iv; wt[w] = it; }
        __syncthreads();
        uint32_t ov = iv - sv, ot = it - st, tile_v = 0, tile_t = 0;
        for (uint32_t j = 0; j < nw; ++j) {
            if (j < w) { ov += wv[j]; ot += wt[j]; }
            tile_v += wv[j];
            tile_t += wt[j];
        }
        __syncthreads();                             // wv / wt are rewritten by the next tile
        uint64_t pv = cv + ov, pt = ct + ot;
#pragma unroll
        for (int k = 0; k < MC_SCAN_PER_THREAD; ++k) {
            if (j0 + k < nblk) sums[j0 + k] = make_uint2((uint32_t)pv, (uint32_t)pt);
            pv += e[k].x;
            pt += e[k].y;
        }
        cv += tile_v;
        ct += tile_t;
    }
}

}  // namespace
