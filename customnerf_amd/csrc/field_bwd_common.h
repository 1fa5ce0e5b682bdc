// Fused field backward (gfx950 matrix cores), two launches:
//   k_field_bwd_data  per 32-sample tile: recompute the forward (nothing was saved), run the activation-gradient chain
//                     dz_l = (W_{l+1}^T dz_{l+1}) * relu'(.) with the C-register trick of field_common.h (transposed weight
//                     fragments, again no cross-lane traffic), write d(loss)/d(grid features) in the encoder's [L,P,2]
//                     layout, and spill every dz_l / layer input once as [row][sample] matrices;
//   k_field_bwd_dw    dW_l = dz_l . a_{l-1}^T : MFMA GEMMs whose contraction runs over the samples, reading those
//                     [row][sample] matrices with 16-byte per-lane loads; split-K over the sample axis, per-workgroup LDS
//                     reduction, one partial row per split (plain stores), summed in a fixed order by k_field_reduce_partials,
//                     which also raises found_inf.
// trunc_exp backward clamps the exponent to [-15, 15] (provider_utils.py:26-29).
#pragma once
#include "field_common.h"

// Weight staging, fragment loads, the layer product, zeroing and the grid-feature load are the forward's (fld_*, field_common.h).

// The forward-order layer product of the backward kernels that run near the register limit (k_field_bwd_data, k_field_bwd_fused, k_mlp_*):
// fld_gemm behind a scheduling fence that keeps this layer's fragment loads from being hoisted above the previous layer
template <bool H, int T, int NS>
__device__ __forceinline__ void fb_gemm(const typename Prec<H>::elem_t *wf, uint32_t S, uint32_t s0, const typename Prec<H>::frag_t *b, uint32_t lane,
                                        cn_f16v (&acc)[T]) {
    asm volatile("" ::: "memory");
    fld_gemm<H, T, NS>(wf, S, s0, b, lane, acc);
}

// transposed staging: A fragment of W^T.  tile t runs over the layer's INPUT features (col0 + 32 t + i), the K-slots over its
// OUTPUT rows in C-register order: dst[((t S + s) 64 + lane) J + j] = W[clayout(s, hi, j)][col0 + 32 t + (lane & 31)]
template <bool H>
__device__ __forceinline__ void fb_stage_layer_T(typename Prec<H>::elem_t *dst, const float *__restrict__ W, uint32_t rows, uint32_t in_stride,
                                                 uint32_t col0, uint32_t n_in, uint32_t T, uint32_t S) {
    using P = Prec<H>;
    const uint32_t total = T * S * 64 * P::J;
    for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
        const uint32_t j = i % P::J, lane = (i / P::J) % 64, ts = i / (P::J * 64);
        const uint32_t s = ts % S, t = ts / S;
        const uint32_t col = 32 * t + (lane & 31), hi = lane >> 5;
        const uint32_t row = (uint32_t)fld_col_clayout<H>(s, hi, j);
        float v = 0.0f;
        if (row < rows && col < n_in) v = W[(size_t)row * in_stride + col0 + col];
        dst[i] = (typename P::elem_t)v;
    }
}

// transposed A fragment straight from the row-major float32 parameters (fp32 mode: no LDS room for a second copy;
// lanes i read consecutive columns -> coalesced)
__device__ __forceinline__ float fb_frag_T_global(const float *__restrict__ W, uint32_t rows, uint32_t in_stride, uint32_t col0, uint32_t n_in,
                                                  uint32_t t, uint32_t s, uint32_t lane) {
    const uint32_t col = 32 * t + (lane & 31), hi = lane >> 5;
    const uint32_t row = (uint32_t)fld_col_clayout<false>(s, hi, 0);
    return (row < rows && col < n_in) ? W[(size_t)row * in_stride + col0 + col] : 0.0f;
}

// da[t] += W^T(t, s) dz[s]   — one transposed layer product
template <bool H, int T, int NS>
__device__ __forceinline__ void fb_gemm_T(const typename Prec<H>::elem_t *wt_lds, const float *__restrict__ W, uint32_t rows, uint32_t in_stride,
                                          uint32_t col0, uint32_t n_in, uint32_t S, const typename Prec<H>::frag_t *b, uint32_t lane, cn_f16v (&acc)[T]) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int t = 0; t < T; t++) {
            typename Prec<H>::frag_t a;
            if constexpr (H) a = fld_load_frag<H>(wt_lds, t, S, s, lane);
            else a = fb_frag_T_global(W, rows, in_stride, col0, n_in, t, s, lane);
            acc[t] = Prec<H>::mfma(a, b[s], acc[t]);
        }
    }
}

// C registers -> next layer's B fragments, the backward's form (k_field_bwd_data, k_field_bwd_fused, k_mlp_*): fmaxf on the accumulators, then
// convert.  Same values as fld_c_to_b (field.hip), other instructions: swapping them changes the kernels' instruction streams.
template <bool H, bool RELU>
__device__ __forceinline__ void fb_c_to_b(const cn_f16v (&acc)[2], typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
#pragma unroll
    for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int sub = 0; sub < P::FR; sub++) {
            if constexpr (H) {
                cn_h8 f;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    float v = acc[u][8 * sub + j];
                    if (RELU) v = fmaxf(v, 0.0f);
                    f[j] = (_Float16)v;
                }
                b[u * P::FR + sub] = f;
            } else {
                float v = acc[u][sub];
                if (RELU) v = fmaxf(v, 0.0f);
                b[u * P::FR + sub] = v;
            }
        }
    }
}

// dz = da * [act > 0]   (act = the forward's post-ReLU fragments, same register mapping as the C tiles)
// (compare and select per half; x4_c_to_b_masked of field_bwd_x2.hip is the packed-integer form of k_field_bwd_x2)
template <bool H>
__device__ __forceinline__ void fb_c_to_b_masked(const cn_f16v (&acc)[2], const typename Prec<H>::frag_t *act, typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
#pragma unroll
    for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int sub = 0; sub < P::FR; sub++) {
            if constexpr (H) {
                cn_h8 f;
                const cn_h8 a = act[u * P::FR + sub];
#pragma unroll
                for (int j = 0; j < 8; j++) f[j] = (a[j] > (_Float16)0) ? (_Float16)acc[u][8 * sub + j] : (_Float16)0;
                b[u * P::FR + sub] = f;
            } else {
                b[u * P::FR + sub] = (act[u * P::FR + sub] > 0.0f) ? acc[u][sub] : 0.0f;
            }
        }
    }
}

// spill 64 rows held as C-ordered B fragments into a [row][sample] matrix (row stride ld)
template <bool H>
__device__ __forceinline__ void fb_dump_clayout(typename Prec<H>::elem_t *__restrict__ M, size_t ld, uint32_t p, uint32_t hi, const typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
#pragma unroll
    for (int s = 0; s < 2 * P::FR; s++) {
#pragma unroll
        for (int j = 0; j < P::J; j++) {
            const int row = fld_col_clayout<H>(s, hi, j);
            if constexpr (H) M[(size_t)row * ld + p] = b[s][j];
            else M[(size_t)row * ld + p] = b[s];
        }
    }
}

// spill natural-ordered fragments (grid features / direction features): rows < n_rows only
template <bool H, int NS>
__device__ __forceinline__ void fb_dump_natural(typename Prec<H>::elem_t *__restrict__ M, size_t ld, uint32_t p, uint32_t hi, const typename Prec<H>::frag_t *b,
                                                uint32_t n_rows) {
    using P = Prec<H>;
#pragma unroll
    for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int j = 0; j < P::J; j++) {
            const uint32_t row = (uint32_t)fld_col_natural<H>(s, hi, j);
            if (row < n_rows) {
                if constexpr (H) M[(size_t)row * ld + p] = b[s][j];
                else M[(size_t)row * ld + p] = b[s];
            }
        }
    }
}

// direction features of sample p; padded samples give zero fragments (they are spilled)
template <bool H>
__device__ __forceinline__ void fb_dir_frags(const float *__restrict__ dirs, uint32_t dir_group, uint32_t p, bool valid, uint32_t hi,
                                             typename Prec<H>::frag_t *b) {
    float dx = 0, dy = 0, dz = 0;
    if (valid) {
        const float *d = dirs + (size_t)(p / dir_group) * 3;
        dx = d[0]; dy = d[1]; dz = d[2];
    }
    fld_dir_frags_from<H>(dx, dy, dz, valid, hi, b);
}

// LDS layout of the backward kernel: forward fragment stores (as field.hip) then the transposed stores (fp16 only)
struct FieldLdsT {
    uint32_t off[8];   // n0T, n1T, n2T, d0T, doT, r0T, roT, end   (elements, relative to the transposed area)
};
template <bool H>
__host__ __device__ __forceinline__ FieldLdsT fb_ldsT_layout(const FieldDims &d) {
    FieldLdsT l;
    const uint32_t t0 = (d.enc_pad + 31) / 32;
    uint32_t o = 0;
    l.off[0] = o; o += 32 * t0 * FLD_HID;                                    // n0T: t0 tiles x K=64
    l.off[1] = o; o += (d.n_hidden_geo == 2) ? FLD_HID * FLD_HID : 0;
    l.off[2] = o; o += FLD_HID * FLD_HID;
    l.off[3] = o; o += FLD_HID * FLD_HID;
    l.off[4] = o; o += FLD_HID * 32;                                         // doT: 2 tiles x K=32
    l.off[5] = o; o += FLD_HID * FLD_HID;                                    // r0T (fea columns only)
    l.off[6] = o; o += FLD_HID * 32;
    l.off[7] = o;
    return l;
}


// Flat [net | den | rgb] parameter space of the partial weight-gradient rows: one layout for every backward form that reduces partials with
// k_field_reduce_partials (the four-wave kernel of field_bwd_fused.hip, k_field_bwd_x2 and the split-K GEMM of field_bwd.hip)
struct FfOff {
    uint32_t n0, n1, n2, d0, dO, r0, rO, total;
};
__host__ __device__ __forceinline__ FfOff ff_offsets(const FieldDims &dm) {
    FfOff o;
    uint32_t p = 0;
    o.n0 = p; p += FLD_HID * dm.enc_pad;
    o.n1 = p; p += (dm.n_hidden_geo == 2) ? 4096 : 0;
    o.n2 = p; p += 4096;
    o.d0 = p; p += 4096;
    o.dO = p; p += 16 * 64;
    o.r0 = p; p += 64 * 96;
    o.rO = p; p += 16 * 64;
    o.total = p;
    return o;
}

// ---- host functions that cross translation units (each defining file includes this header and so sees the declaration it implements)
// field_bwd_fused.hip: g += sum of the partial rows (fixed order, raises found_inf); the single-launch fp16 form
void ff_reduce_partials(const float *partials, uint32_t n_partials, uint32_t total, uint32_t n_net, uint32_t n_den, float *g_net, float *g_den, float *g_rgb,
                        hipStream_t st);
uint64_t ff_workspace_bytes(const FieldDims &dm);
int ff_launch(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P_, const FieldDims &dm, const float *pnet,
              const float *pden, const float *prgb, const float *g_sigma, const float *g_rgbc, void *grad_enc, float *g_net, float *g_den,
              float *g_rgb, void *workspace, const uint8_t *tile_live, hipStream_t st, const void *wimg);
// field_bwd_x2.hip: the two-pipeline kernel for 32-wide encodings (9..16 levels); the four-wave kernel of field_bwd_fused.hip serves the narrower ones
bool x2_eligible(const FieldDims &dm);
int x2_launch(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P_, const FieldDims &dm, const float *pnet, const float *pden,
              const float *prgb, const float *g_sigma, const float *g_rgbc, void *grad_enc, float *g_net, float *g_den, float *g_rgb, void *workspace,
              uint32_t max_partials, const uint8_t *tile_live, hipStream_t st, const void *wimg);
