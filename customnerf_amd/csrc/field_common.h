// Fused NeRF field (grid features -> sigma / rgb MLPs) on the gfx950 matrix cores: shared definitions.
//
// The three bias-free MLPs of nerf/network_grid.py:98-139 are evaluated per 32-sample tile by one wavefront with
// v_mfma_f32_32x32x16_f16 (fp16 mode: tinycudann FullyFusedMLP numerics) or v_mfma_f32_32x32x2_f32 (fp32 mode: exact
// float32, same rate as the vector ALU but with the same data flow).  Orientation: Y[out, sample] = W[out, k] X[k, sample]:
// A = weights (from LDS, pre-arranged in fragment order), B = activations, C = 32 outputs x 32 samples.
//
// Key layout fact (CDNA4 MFMA): lane l of a wave owns sample (l & 31); for a C tile it holds output rows
//   rho(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi,  r = 0..15, hi = l >> 5,
// and for a B fragment it holds K-slots (hi, j).  Since the contraction index can be permuted freely as long as A and B
// agree, the next layer takes the C registers of the previous one *as they are* as its B fragments (K-slot (s, hi, j) :=
// feature 32 u + rho(r, hi) with r = (s mod FR) J + j, u = s / FR) and the weight fragments are staged into LDS in that
// permuted column order once per workgroup.  No cross-lane traffic between layers.
#pragma once
#include <type_traits>
#include "common.h"

typedef _Float16 cn_h8 __attribute__((ext_vector_type(8)));
typedef _Float16 cn_h2 __attribute__((ext_vector_type(2)));
typedef float cn_f16v __attribute__((ext_vector_type(16)));

#define FLD_THREADS 256
#define FLD_WAVES 4
#define FLD_TILE 32                 // samples per wave tile
#define FLD_HID 64                  // hidden width (the only width the reference uses)
#define FLD_DIR 32                  // 27 frequency features of the view direction, padded to 32
#define FLD_NDIR 27

template <bool HALF> struct Prec;
template <> struct Prec<true> {
    using elem_t = _Float16;
    using frag_t = cn_h8;
    static constexpr int KS = 16;   // k consumed per MFMA
    static constexpr int J = 8;     // elements per lane per fragment
    static constexpr int FR = 2;    // B fragments one 32-row C tile turns into
    static __device__ __forceinline__ cn_f16v mfma(frag_t a, frag_t b, cn_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ frag_t zero() { return frag_t{0, 0, 0, 0, 0, 0, 0, 0}; }
};
template <> struct Prec<false> {
    using elem_t = float;
    using frag_t = float;
    static constexpr int KS = 2;
    static constexpr int J = 1;
    static constexpr int FR = 16;
    static __device__ __forceinline__ cn_f16v mfma(frag_t a, frag_t b, cn_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ frag_t zero() { return 0.0f; }
};

__host__ __device__ __forceinline__ int fld_rho(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// feature index of K-slot (s, hi, j) for activations that arrive in C-register order / in natural order
template <bool H> __host__ __device__ __forceinline__ int fld_col_clayout(int s, int hi, int j) {
    const int u = s / Prec<H>::FR, r = (s % Prec<H>::FR) * Prec<H>::J + j;
    return 32 * u + fld_rho(r, hi);
}
template <bool H> __host__ __device__ __forceinline__ int fld_col_natural(int s, int hi, int j) { return Prec<H>::KS * s + Prec<H>::J * hi + j; }

// Network geometry (all widths in elements)
struct FieldDims {
    uint32_t enc_dim;        // L * C (<= 64)
    uint32_t enc_pad;        // padded to x16
    uint32_t n_hidden_geo;   // 1 or 2 hidden layers in `network`
    uint32_t n_rgb_out;      // 3 or 4
    uint32_t L;              // levels (enc_dim / 2)
};

// LDS fragment-store offsets (in elements) of the seven layers: n0, n1, n2, d0, do, r0, ro
struct FieldLds {
    uint32_t off[8];
};

template <bool H>
__host__ __device__ __forceinline__ FieldLds fld_lds_layout(const FieldDims &d) {
    FieldLds l;
    uint32_t o = 0;
    l.off[0] = o; o += FLD_HID * d.enc_pad;                              // n0  [64, enc_pad]
    l.off[1] = o; o += (d.n_hidden_geo == 2) ? FLD_HID * FLD_HID : 0;    // n1  [64, 64]
    l.off[2] = o; o += FLD_HID * FLD_HID;                                // n2  [64, 64]
    l.off[3] = o; o += FLD_HID * FLD_HID;                                // d0  [64, 64]
    l.off[4] = o; o += 32 * FLD_HID;                                     // do  one 32-row tile (16 parameter rows + zeros)
    l.off[5] = o; o += FLD_HID * (FLD_HID + FLD_DIR);                    // r0  [64, 64 fea + 32 dir]
    l.off[6] = o; o += 32 * FLD_HID;                                     // ro
    l.off[7] = o;
    return l;
}

// Direction features of a 32-sample tile whose samples share ONE direction (dir_group a multiple of the tile: the renderer's run() path,
// one direction per ray).  Instead of every lane evaluating all 24 sines / cosines, lane q < 27 evaluates feature q, the 32 halves go
// through a 64-byte LDS scratch of the wave and come back as the two natural-order B fragments (broadcast reads).  `scratch` must be
// 16-byte aligned and private to the wave; DS operations of one wave execute in order, no barrier is involved.
__device__ __forceinline__ void fld_dir_frags_uniform(float dx, float dy, float dz, uint32_t lane, uint32_t hi, unsigned char *scratch, cn_h8 *b) {
    const uint32_t q = lane & 31;
    const uint32_t qq = q >= 3 ? q - 3 : 0, k = qq / 6, r = qq % 6, c = q < 3 ? q : (r < 3 ? r : r - 3);
    const float d = c == 0 ? dx : (c == 1 ? dy : dz);
    const float a = d * (float)(1u << k);
    const float sc = r < 3 ? __sinf(a) : __cosf(a);
    const float v = q < 3 ? d : (q < FLD_NDIR ? sc : 0.0f);
    if (lane < 32) reinterpret_cast<_Float16 *>(scratch)[q] = (_Float16)v;
    b[0] = *reinterpret_cast<const cn_h8 *>(scratch + 16 * hi);
    b[1] = *reinterpret_cast<const cn_h8 *>(scratch + 32 + 16 * hi);
}

// frequency encoding of a direction (nerf/base.py:42-60): [d, sin(2^k d), cos(2^k d)]_{k=0..3}, 27 values padded to 32
template <bool FAST>
__device__ __forceinline__ void fld_dir_features(float dx, float dy, float dz, float (&e)[FLD_DIR]) {
    const float d[3] = {dx, dy, dz};
#pragma unroll
    for (int c = 0; c < 3; c++) e[c] = d[c];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float f = (float)(1 << k);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float s, co;
            if (FAST) { s = __sinf(d[c] * f); co = __cosf(d[c] * f); }
            else { s = sinf(d[c] * f); co = cosf(d[c] * f); }
            e[3 + 6 * k + c] = s;
            e[6 + 6 * k + c] = co;
        }
    }
#pragma unroll
    for (int q = FLD_NDIR; q < FLD_DIR; q++) e[q] = 0.0f;
}

// direction -> its 32 features -> the natural-order B fragments of the colour layer's direction columns.  `keep` false zeroes them: the backward
// spills the fragments of padded samples and must spill zeros (cos(0) = 1 otherwise); the forward, which stores nothing for them, passes true
template <bool H>
__device__ __forceinline__ void fld_dir_frags_from(float dx, float dy, float dz, bool keep, uint32_t hi, typename Prec<H>::frag_t *b) {
    float e[FLD_DIR];
    fld_dir_features<H>(dx, dy, dz, e);
    if (!keep) {
#pragma unroll
        for (int q = 0; q < FLD_DIR; q++) e[q] = 0.0f;
    }
    if constexpr (H) {
#pragma unroll
        for (int s = 0; s < FLD_DIR / 16; s++) {
            cn_h8 f;
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = (_Float16)(hi ? e[16 * s + 8 + j] : e[16 * s + j]);
            b[s] = f;
        }
    } else {
#pragma unroll
        for (int s = 0; s < FLD_DIR / 2; s++) b[s] = hi ? e[2 * s + 1] : e[2 * s];
    }
}

// ------------------------------------------------------------------------------------------------ weight staging
// Copy one layer's [rows, in_stride] float32 matrix into LDS in A-fragment order:
//   dst[((t * S + s) * 64 + lane) * J + j] = W[32 t + (lane & 31)][col(s, lane >> 5, j)]      (0 where out of range)
// KIND 0: natural column order (grid features).  KIND 1: C-register order (hidden activations).
// KIND 2: rgb layer 0 = [C-ordered fea at column 27.., then natural dir features at column 0..26].
// The caller's threads cover element indices i0, i0 + istride, ...: a workgroup staging into its LDS passes (threadIdx.x, its thread
// count), k_field_pack spreads one image over a whole grid.
// SWZ: 16-byte fragment slots bank-swizzled for the transposing reads of field_bwd_x2.hip
// (slot bits 2..3 ^= (K-step parity, half) — halves index i, i.e. byte offset 2 i; needs an even S)
template <bool H, int KIND, bool SWZ = false>
__device__ __forceinline__ void fld_stage_layer(typename Prec<H>::elem_t *dst, const float *__restrict__ W, uint32_t rows, uint32_t in_stride,
                                                uint32_t T, uint32_t S, uint32_t n_valid_cols, uint32_t i0, uint32_t istride) {
    using P = Prec<H>;
    const uint32_t total = T * S * 64 * P::J;
    for (uint32_t i = i0; i < total; i += istride) {
        const uint32_t j = i % P::J, lane = (i / P::J) % 64, ts = i / (P::J * 64);
        const uint32_t s = ts % S, t = ts / S;
        const uint32_t row = 32 * t + (lane & 31), hi = lane >> 5;
        int col;
        if (KIND == 0) col = fld_col_natural<H>(s, hi, j);
        else if (KIND == 1) col = fld_col_clayout<H>(s, hi, j);
        else {
            const uint32_t s_fea = FLD_HID / P::KS;
            if (s < s_fea) col = FLD_NDIR + fld_col_clayout<H>(s, hi, j);
            else {
                col = fld_col_natural<H>(s - s_fea, hi, j);
                if (col >= FLD_NDIR) col = -1;
            }
        }
        float v = 0.0f;
        if (row < rows && col >= 0 && (uint32_t)col < n_valid_cols) v = W[(size_t)row * in_stride + col];
        dst[SWZ ? (i ^ (((i >> 8) & 3u) << 5)) : i] = (typename P::elem_t)v;
    }
}

// The same fragment order for the TRANSPOSE of a layer whose 64 outputs arrive in C-register order (a gradient running back through it,
// field_normal.hip): A(row, k) = W[col(k)][row] with W the layer's [64, in_stride] matrix, row = one of its `n_in` inputs (0 beyond),
// k = its outputs in the column order of KIND 1.  T = tiles of 32 inputs, S = FLD_HID / KS.
template <bool H>
__device__ __forceinline__ void fld_stage_layer_t(typename Prec<H>::elem_t *dst, const float *__restrict__ W, uint32_t n_in, uint32_t in_stride,
                                                  uint32_t T, uint32_t S, uint32_t i0, uint32_t istride) {
    using P = Prec<H>;
    const uint32_t total = T * S * 64 * P::J;
    for (uint32_t i = i0; i < total; i += istride) {
        const uint32_t j = i % P::J, lane = (i / P::J) % 64, ts = i / (P::J * 64);
        const uint32_t s = ts % S, t = ts / S;
        const uint32_t row = 32 * t + (lane & 31), hi = lane >> 5;
        const uint32_t col = (uint32_t)fld_col_clayout<H>(s, hi, j);
        float v = 0.0f;
        if (row < n_in && col < FLD_HID) v = W[(size_t)col * in_stride + row];
        dst[i] = (typename P::elem_t)v;
    }
}

// ------------------------------------------------------------------------------------------------ per-wave building blocks
template <bool H>
__device__ __forceinline__ typename Prec<H>::frag_t fld_load_frag(const typename Prec<H>::elem_t *base, uint32_t t, uint32_t S, uint32_t s, uint32_t lane) {
    using P = Prec<H>;
    return *reinterpret_cast<const typename P::frag_t *>(base + ((size_t)(t * S + s) * 64 + lane) * P::J);
}

// acc[t] = sum_s A(t, s) * b[s]    for t < T, s in [s0, s0 + NS) of a layer whose fragment store has S K-steps per tile
template <bool H, int T, int NS>
__device__ __forceinline__ void fld_gemm(const typename Prec<H>::elem_t *wf, uint32_t S, uint32_t s0, const typename Prec<H>::frag_t *b, uint32_t lane,
                                         cn_f16v (&acc)[T]) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int t = 0; t < T; t++) acc[t] = Prec<H>::mfma(fld_load_frag<H>(wf, t, S, s0 + s, lane), b[s], acc[t]);
    }
}

template <int T>
__device__ __forceinline__ void fld_zero(cn_f16v (&acc)[T]) {
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
}

// grid features of one sample as B fragments (natural order): lane (p, hi) reads levels per K-step from enc [L, P, 2]
template <bool H, int SENC>
__device__ __forceinline__ void fld_load_enc(const void *__restrict__ enc, uint32_t P_, uint32_t L, uint32_t p, bool valid, uint32_t hi,
                                             typename Prec<H>::frag_t (&b)[SENC]) {
    if constexpr (H) {
        const uint32_t *e = reinterpret_cast<const uint32_t *>(enc);      // one half2 per (level, sample)
#pragma unroll
        for (int s = 0; s < SENC; s++) {
            union { cn_h8 h; uint32_t u[4]; } f;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const uint32_t level = 8 * s + 4 * hi + jj;
                f.u[jj] = (valid && level < L) ? e[(size_t)level * P_ + p] : 0u;
            }
            b[s] = f.h;
        }
    } else {
        const float *e = reinterpret_cast<const float *>(enc);
#pragma unroll
        for (int s = 0; s < SENC; s++) {
            const uint32_t feat = 2 * s + hi, level = feat >> 1;          // K-step s holds features (2s, 2s+1) = (level s, c = hi)
            b[s] = (valid && level < L) ? e[((size_t)level * P_ + p) * 2 + (feat & 1)] : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// shape check of the C entry points -> network geometry
static inline int fld_dims(uint32_t enc_dim, uint32_t n_hidden_geo, uint32_t n_rgb_out, FieldDims &dm) {
    if (enc_dim == 0 || enc_dim > 64 || (enc_dim & 1)) return CNERF_EINVAL;
    if (n_hidden_geo < 1 || n_hidden_geo > 2) return CNERF_EINVAL;
    if (n_rgb_out != 3 && n_rgb_out != 4) return CNERF_EINVAL;
    dm.enc_dim = enc_dim;
    dm.enc_pad = (enc_dim + 15) / 16 * 16;
    dm.n_hidden_geo = n_hidden_geo;
    dm.n_rgb_out = n_rgb_out;
    dm.L = enc_dim / 2;
    return CNERF_OK;
}

// The kernels are instantiated per (enc_pad / 16 = 1..4, hidden layers of `network` = 1 | 2): calls f with the two as integral constants,
// false for any other shape
template <int NG, class F>
static inline bool fld_dispatch_ng(uint32_t se16, F &f) {
    switch (se16) {
        case 1: f(std::integral_constant<int, 1>(), std::integral_constant<int, NG>()); return true;
        case 2: f(std::integral_constant<int, 2>(), std::integral_constant<int, NG>()); return true;
        case 3: f(std::integral_constant<int, 3>(), std::integral_constant<int, NG>()); return true;
        case 4: f(std::integral_constant<int, 4>(), std::integral_constant<int, NG>()); return true;
        default: return false;
    }
}
template <class F>
static inline bool fld_dispatch(const FieldDims &dm, F f) {
    return dm.n_hidden_geo == 1 ? fld_dispatch_ng<1>(dm.enc_pad / 16, f) : fld_dispatch_ng<2>(dm.enc_pad / 16, f);
}
