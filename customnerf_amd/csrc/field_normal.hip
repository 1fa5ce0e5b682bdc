// Field normals: the analytic gradient of the log-density with respect to position, in three kernels.
//   sigma = exp(raw(x) + blob(x)),  raw = MLP_den(MLP_net(enc(x)))[0]   =>   normal direction = -grad_x(raw + blob)
//   k_field_density_grad   d raw / d enc     one backward pass through the two bias-free ReLU MLPs with a 1 as the upstream gradient
//   k_grid_input_grad      d enc / d x       the trilinear derivative of the table, contracted with d raw / d enc (no dy_dx is written)
//   k_composite_normals    sum_s w n, sum_s w max(0, n . d)^2 per ray   (renderer.py:428, :469-470)
// The blob's gradient and the unit-cube scaling are two elementwise steps of the caller (nerf/network_grid.py: density_gradient).
#include "field_common.h"
#include "grid_common.h"

// ------------------------------------------------------------------------------------------------ d raw / d enc
// Data flow of k_field_fwd (field.hip), per 32-sample tile of one wave: the forward is recomputed with the ReLU masks kept as one bit per
// C register (32 per layer and lane), then the gradient runs back through the TRANSPOSED weight fragments (fld_stage_layer_t).  A gradient
// vector is born in the C-register order of the layer it leaves, which is the B-fragment order of the transposed layer before it — the
// same "C registers are the next B fragments" rule as the forward, so no cross-lane traffic here either.
//
// LDS: the forward's five layers + the four transposed ones + row 0 of the output layer.  Largest instantiation (float32, 64 features,
// two hidden layers): 18432 + 16384 + 64 floats = 136.25 KiB of the CU's 160 KiB: one workgroup per CU; half precision takes 68.1 KiB: two.
struct FieldNormalLds {
    uint32_t d0t, n2t, n1t, n0t, wout, end;       // element offsets behind the forward's layers (FieldLds::off[5])
    uint32_t t_enc;                               // 32-row tiles of the transposed first layer
};
template <bool H>
__host__ __device__ __forceinline__ FieldNormalLds fn_lds_layout(const FieldDims &d) {
    FieldNormalLds l;
    uint32_t o = fld_lds_layout<H>(d).off[5];
    l.t_enc = (d.enc_pad + 31) / 32;
    l.d0t = o; o += FLD_HID * FLD_HID;
    l.n2t = o; o += FLD_HID * FLD_HID;
    l.n1t = o; o += (d.n_hidden_geo == 2) ? FLD_HID * FLD_HID : 0;
    l.n0t = o; o += l.t_enc * 32 * FLD_HID;
    l.wout = o; o += FLD_HID;
    l.end = o;
    return l;
}

// C registers of two 32-row tiles -> the B fragments of the next layer through ReLU, values as fld_c_to_b<H, true> gives them (fp16 mode
// rounds first: rounding keeps the sign); bit (s J + j) of the returned mask says that element j of fragment s is alive
template <bool H>
__device__ __forceinline__ uint32_t fn_relu_to_b(const cn_f16v (&acc)[2], typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
    uint32_t mask = 0;
#pragma unroll
    for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int sub = 0; sub < P::FR; sub++) {
            const int s = u * P::FR + sub;
            if constexpr (H) {
                cn_h8 f;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const _Float16 v = (_Float16)acc[u][8 * sub + j];
                    const bool on = v > (_Float16)0;
                    mask |= (uint32_t)on << (8 * s + j);
                    f[j] = on ? v : (_Float16)0;
                }
                b[s] = f;
            } else {
                const float v = acc[u][sub];
                const bool on = v > 0.0f;
                mask |= (uint32_t)on << s;
                b[s] = on ? v : 0.0f;
            }
        }
    }
    return mask;
}
// ... without activation (the output of `network`)
template <bool H>
__device__ __forceinline__ void fn_to_b(const cn_f16v (&acc)[2], typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
#pragma unroll
    for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int sub = 0; sub < P::FR; sub++) {
            if constexpr (H) {
                cn_h8 f;
#pragma unroll
                for (int j = 0; j < 8; j++) f[j] = (_Float16)acc[u][8 * sub + j];
                b[u * P::FR + sub] = f;
            } else {
                b[u * P::FR + sub] = acc[u][sub];
            }
        }
    }
}
// a gradient in C registers -> the B fragments of the transposed layer before it, through the ReLU mask of the activation it belongs to
// (fp16 mode rounds the gradient to half here, as the activations are between the forward's layers)
template <bool H, bool MASKED>
__device__ __forceinline__ void fn_grad_to_b(const cn_f16v (&acc)[2], uint32_t mask, typename Prec<H>::frag_t *b) {
    using P = Prec<H>;
#pragma unroll
    for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int sub = 0; sub < P::FR; sub++) {
            const int s = u * P::FR + sub;
            if constexpr (H) {
                cn_h8 f;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const bool on = !MASKED || ((mask >> (8 * s + j)) & 1u);
                    f[j] = on ? (_Float16)acc[u][8 * sub + j] : (_Float16)0;
                }
                b[s] = f;
            } else {
                const bool on = !MASKED || ((mask >> s) & 1u);
                b[s] = on ? acc[u][sub] : 0.0f;
            }
        }
    }
}

__device__ __forceinline__ float fn_round_half(float v) { return (float)(_Float16)v; }

template <bool H, int SENC, int NGEO>
__global__ void __launch_bounds__(FLD_THREADS, H ? 2 : 1) k_field_density_grad(const void *__restrict__ enc, const float *__restrict__ xyz, uint32_t P_,
                                                                                FieldDims dm, const float *__restrict__ pnet,
                                                                                const float *__restrict__ pden, float *__restrict__ sigma,
                                                                                float *__restrict__ grad_enc, uint32_t enc_stride) {
    using PR = Prec<H>;
    using frag_t = typename PR::frag_t;
    using elem_t = typename PR::elem_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char fn_lds[];
    elem_t *wl = reinterpret_cast<elem_t *>(fn_lds);
    const FieldLds lo = fld_lds_layout<H>(dm);
    const FieldNormalLds ln = fn_lds_layout<H>(dm);
    constexpr uint32_t S64 = FLD_HID / PR::KS;
    constexpr int TENC = (SENC * PR::KS + 31) / 32;
    {
        const float *n0 = pnet, *n1 = pnet + FLD_HID * dm.enc_pad;
        const float *n2 = n1 + (NGEO == 2 ? FLD_HID * FLD_HID : 0);
        const float *wo = pden + FLD_HID * FLD_HID;
        const uint32_t i0 = threadIdx.x;
        fld_stage_layer<H, 0>(wl + lo.off[0], n0, FLD_HID, dm.enc_pad, 2, SENC, dm.enc_pad, i0, FLD_THREADS);
        if (NGEO == 2) fld_stage_layer<H, 1>(wl + lo.off[1], n1, FLD_HID, FLD_HID, 2, S64, FLD_HID, i0, FLD_THREADS);
        fld_stage_layer<H, 1>(wl + lo.off[2], n2, FLD_HID, FLD_HID, 2, S64, FLD_HID, i0, FLD_THREADS);
        fld_stage_layer<H, 1>(wl + lo.off[3], pden, FLD_HID, FLD_HID, 2, S64, FLD_HID, i0, FLD_THREADS);
        fld_stage_layer<H, 1>(wl + lo.off[4], wo, 16, FLD_HID, 1, S64, FLD_HID, i0, FLD_THREADS);
        fld_stage_layer_t<H>(wl + ln.d0t, pden, FLD_HID, FLD_HID, 2, S64, i0, FLD_THREADS);
        fld_stage_layer_t<H>(wl + ln.n2t, n2, FLD_HID, FLD_HID, 2, S64, i0, FLD_THREADS);
        if (NGEO == 2) fld_stage_layer_t<H>(wl + ln.n1t, n1, FLD_HID, FLD_HID, 2, S64, i0, FLD_THREADS);
        fld_stage_layer_t<H>(wl + ln.n0t, n0, dm.enc_dim, dm.enc_pad, TENC, S64, i0, FLD_THREADS);
        if (i0 < FLD_HID) wl[ln.wout + i0] = (elem_t)wo[i0];          // row 0 of the output layer: d raw / d (its input)
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hi = lane >> 5;
    const uint32_t n_tiles = (P_ + FLD_TILE - 1) / FLD_TILE;
    for (uint32_t tile = blockIdx.x * FLD_WAVES + wave; tile < n_tiles; tile += gridDim.x * FLD_WAVES) {
        asm volatile("" ::: "memory");           // keep the weight fragments in LDS (see k_field_fwd)
        const uint32_t p = tile * FLD_TILE + (lane & 31);
        const bool valid = p < P_;

        // ---- the forward, as k_field_fwd computes it
        frag_t x0[SENC];
        fld_load_enc<H, SENC>(enc, enc_stride, dm.L, p, valid, hi, x0);
        cn_f16v acc[2];
        frag_t h[2 * PR::FR];
        uint32_t m0, m1 = 0;
        fld_zero(acc);
        fld_gemm<H, 2, SENC>(wl + lo.off[0], SENC, 0, x0, lane, acc);
        m0 = fn_relu_to_b<H>(acc, h);
        if (NGEO == 2) {
            fld_zero(acc);
            fld_gemm<H, 2, S64>(wl + lo.off[1], S64, 0, h, lane, acc);
            m1 = fn_relu_to_b<H>(acc, h);
        }
        fld_zero(acc);
        fld_gemm<H, 2, S64>(wl + lo.off[2], S64, 0, h, lane, acc);
        fn_to_b<H>(acc, h);
        fld_zero(acc);
        fld_gemm<H, 2, S64>(wl + lo.off[3], S64, 0, h, lane, acc);
        const uint32_t md = fn_relu_to_b<H>(acc, h);
        if (sigma) {
            cn_f16v out[1];
            fld_zero(out);
            fld_gemm<H, 1, S64>(wl + lo.off[4], S64, 0, h, lane, out);
            if (valid && hi == 0) {
                float raw = out[0][0];
                if (H) raw = fn_round_half(raw);
                const float x = xyz[(size_t)p * 3], y = xyz[(size_t)p * 3 + 1], z = xyz[(size_t)p * 3 + 2];
                const float g = H ? 5.0f * __expf(-(x * x + y * y + z * z) * (1.0f / 0.08f)) : 5.0f * expf(-(x * x + y * y + z * z) / 0.08f);
                sigma[p] = H ? __expf(raw + g) : expf(raw + g);
            }
        }

        // ---- the gradient: g_hd = w_out[0, :] (.) mask_d, in the C-register order of the density head's hidden layer
#pragma unroll
        for (int s = 0; s < 2 * PR::FR; s++) {
            if constexpr (H) {
                cn_h8 f;
#pragma unroll
                for (int j = 0; j < 8; j++) f[j] = ((md >> (8 * s + j)) & 1u) ? wl[ln.wout + fld_col_clayout<H>(s, hi, j)] : (_Float16)0;
                h[s] = f;
            } else {
                h[s] = ((md >> s) & 1u) ? wl[ln.wout + fld_col_clayout<H>(s, hi, 0)] : 0.0f;
            }
        }
        fld_zero(acc);
        fld_gemm<H, 2, S64>(wl + ln.d0t, S64, 0, h, lane, acc);          // g_fea = W_d0^T g_hd   (fea has no activation)
        fn_grad_to_b<H, false>(acc, 0u, h);
        fld_zero(acc);
        fld_gemm<H, 2, S64>(wl + ln.n2t, S64, 0, h, lane, acc);          // g_h = W_n,last^T g_fea (.) mask
        fn_grad_to_b<H, true>(acc, NGEO == 2 ? m1 : m0, h);
        if (NGEO == 2) {
            fld_zero(acc);
            fld_gemm<H, 2, S64>(wl + ln.n1t, S64, 0, h, lane, acc);
            fn_grad_to_b<H, true>(acc, m0, h);
        }
        cn_f16v ge[TENC];
        fld_zero(ge);
        fld_gemm<H, TENC, S64>(wl + ln.n0t, S64, 0, h, lane, ge);        // g_enc = W_n0^T g_h: rows = grid features 2 level + c
        if (valid) {
#pragma unroll
            for (int t = 0; t < TENC; t++) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const uint32_t level = (uint32_t)(32 * t + fld_rho(r, hi)) >> 1;         // rho(r + 1) = rho(r) + 1 for even r: c = 0, 1
                    if (level < dm.L) *reinterpret_cast<float2 *>(grad_enc + ((size_t)level * P_ + p) * 2) = make_float2(ge[t][r], ge[t][r + 1]);
                }
            }
        }
    }
}

template <bool H>
static int fn_launch_density_grad(const void *enc, const float *xyz, uint32_t P_, const FieldDims &dm, const float *pnet, const float *pden, float *sigma,
                                  float *grad_enc, uint32_t enc_stride, hipStream_t st) {
    const uint32_t lds_bytes = fn_lds_layout<H>(dm).end * sizeof(typename Prec<H>::elem_t);
    uint32_t blocks = cn_div_up(cn_div_up(P_, FLD_TILE), FLD_WAVES);
    const uint32_t max_blocks = H ? 512 : 256;            // persistent: LDS allows 2 (fp16) / 1 (fp32) workgroups per CU
    if (blocks > max_blocks) blocks = max_blocks;
    const bool ok = fld_dispatch(dm, [&](auto se16, auto ng) {
        auto kern = k_field_density_grad<H, se16 * 16 / Prec<H>::KS, ng>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(FLD_THREADS), lds_bytes, st, enc, xyz, P_, dm, pnet, pden, sigma, grad_enc, enc_stride);
    });
    if (!ok) return CNERF_EINVAL;
    return cn_launch_status();
}

// ------------------------------------------------------------------------------------------------ d enc / d x, contracted
// One thread per (sample, level): its 8 corners' rows, the derivative of the trilinear weights, three partial sums.  The 32 level slots of
// a sample meet in LDS and one thread per (sample, axis) adds them in level order: no float atomics, the same bits on every run.
#define FN_GIG_SAMPLES (GE_BLOCK / GE_MAX_LEVELS)
template <typename T>
__global__ void __launch_bounds__(GE_BLOCK) k_grid_input_grad(const float *__restrict__ inputs, const T *__restrict__ table, GridLevels lv,
                                                             const float *__restrict__ grad_enc, uint32_t B, uint32_t L, uint32_t stride,
                                                             uint32_t gridtype, float *__restrict__ grad_inputs) {
    __shared__ float part[FN_GIG_SAMPLES][GE_MAX_LEVELS][3];
    const uint32_t level = threadIdx.x / FN_GIG_SAMPLES, sl = threadIdx.x % FN_GIG_SAMPLES;
    const size_t b = (size_t)blockIdx.x * FN_GIG_SAMPLES + sl;
    float a[3] = {0.0f, 0.0f, 0.0f};
    if (b < B && level < L) {
        float in[3];
        ge_load_coords<3>(inputs, b, in);
        if (ge_in_range<3>(in)) {                                   // outside the unit cube the forward writes zero features
            const float scale = lv.scale[level];
            const uint32_t size = lv.size[level], res = lv.resolution[level];
            uint32_t pg[3];
            float fr[3];
            ge_cell<3>(in, scale, false, pg, fr);
            const float2 g = *reinterpret_cast<const float2 *>(grad_enc + ((size_t)level * stride + b) * 2);
            const FeatVec<T, 2> *tab = reinterpret_cast<const FeatVec<T, 2> *>(table) + lv.offset[level];
#pragma unroll
            for (int idx = 0; idx < 8; idx++) {
                uint32_t pc[3];
                float w[3];
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const bool up = (idx >> d) & 1;
                    pc[d] = pg[d] + (up ? 1u : 0u);
                    w[d] = up ? fr[d] : 1.0f - fr[d];
                }
                const FeatVec<T, 2> f = tab[ge_index<3>(gridtype, false, size, res, pc)];
                const float dot = ge_to_float(f.v[0]) * g.x + ge_to_float(f.v[1]) * g.y;
                a[0] += ((idx & 1) ? dot : -dot) * (w[1] * w[2]);
                a[1] += ((idx & 2) ? dot : -dot) * (w[0] * w[2]);
                a[2] += ((idx & 4) ? dot : -dot) * (w[0] * w[1]);
            }
#pragma unroll
            for (int d = 0; d < 3; d++) a[d] *= scale;               // d frac / d u = the level's scale
        }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) part[sl][level][d] = a[d];          // (level < GE_MAX_LEVELS by the block's shape; slots >= L hold zeros)
    __syncthreads();
    if (threadIdx.x < FN_GIG_SAMPLES * 3) {
        const uint32_t s2 = threadIdx.x / 3, d = threadIdx.x % 3;
        const size_t b2 = (size_t)blockIdx.x * FN_GIG_SAMPLES + s2;
        if (b2 < B) {
            float sum = 0.0f;
            for (uint32_t l = 0; l < L; l++) sum += part[s2][l][d];
            grad_inputs[b2 * 3 + d] = sum;
        }
    }
}

// ------------------------------------------------------------------------------------------------ per-ray normal map and orientation term
// One wave per ray; lane i takes samples i, i + 64, ...; the 64 partial sums meet in a butterfly whose order does not depend on the data.
#define FN_CN_VMAX 3
__global__ void __launch_bounds__(256) k_composite_normals(const float *__restrict__ weights, const int32_t *__restrict__ src_index,
                                                           const float *__restrict__ grad_x, const float *__restrict__ dirs, uint32_t V, uint32_t N,
                                                           uint32_t S, uint32_t P_, float *__restrict__ normal_map, float *__restrict__ orient) {
    const uint32_t lane = threadIdx.x & 63, ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= N) return;                                            // whole waves leave: nothing below synchronises across waves
    const float dx = dirs[(size_t)ray * 3], dy = dirs[(size_t)ray * 3 + 1], dz = dirs[(size_t)ray * 3 + 2];
    float acc[FN_CN_VMAX][4];
#pragma unroll
    for (int v = 0; v < FN_CN_VMAX; v++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[v][k] = 0.0f;
    for (uint32_t i = lane; i < S; i += 64) {
        const size_t pos = (size_t)ray * S + i;
        const size_t row = src_index ? (size_t)(uint32_t)src_index[pos] : pos;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        if (row < P_) {
            const float gx = grad_x[row * 3], gy = grad_x[row * 3 + 1], gz = grad_x[row * 3 + 2];
            const float q = gx * gx + gy * gy + gz * gz;
            if (q >= 1e-20f) {                                       // safe_normalize's epsilon (provider_utils.py:125-126): below it the normal is zero
                const float inv = -1.0f / sqrtf(q);
                nx = gx * inv; ny = gy * inv; nz = gz * inv;
            }
        }
        const float c = fmaxf(nx * dx + ny * dy + nz * dz, 0.0f);
#pragma unroll
        for (int v = 0; v < FN_CN_VMAX; v++) {
            if (v < (int)V) {
                const float w = weights[((size_t)v * N + ray) * S + i];
                acc[v][0] += w * nx; acc[v][1] += w * ny; acc[v][2] += w * nz; acc[v][3] += w * (c * c);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < FN_CN_VMAX; v++) {
        if (v < (int)V) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float x = acc[v][k];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
                acc[v][k] = x;
            }
            if (lane == 0) {
                float *nm = normal_map + ((size_t)v * N + ray) * 3;
                nm[0] = acc[v][0]; nm[1] = acc[v][1]; nm[2] = acc[v][2];
                orient[(size_t)v * N + ray] = acc[v][3];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" {

int cnerf_field_density_grad(const void *enc, const float *xyz, uint32_t P_, uint32_t enc_dim, uint32_t n_hidden_geo, const float *params_net,
                             const float *params_den, float *sigma, float *grad_enc, int dtype, uint32_t enc_level_stride, void *stream) {
    FieldDims dm;
    int rc = fld_dims(enc_dim, n_hidden_geo, 4, dm);
    if (rc) return rc;
    if (dtype != CNERF_F32 && dtype != CNERF_F16) return CNERF_EINVAL;
    if (enc_level_stride == 0) enc_level_stride = P_;
    if (enc_level_stride < P_) return CNERF_EINVAL;
    if (P_ == 0) return CNERF_OK;
    if (!enc || !xyz || !params_net || !params_den || !grad_enc) return CNERF_ENULL;
    if (((uintptr_t)grad_enc) & 7) return CNERF_EINVAL;
    if (dtype == CNERF_F16)
        return fn_launch_density_grad<true>(enc, xyz, P_, dm, params_net, params_den, sigma, grad_enc, enc_level_stride, CN_STREAM(stream));
    return fn_launch_density_grad<false>(enc, xyz, P_, dm, params_net, params_den, sigma, grad_enc, enc_level_stride, CN_STREAM(stream));
}

int cnerf_grid_encode_input_grad(const float *inputs, const void *embeddings, const int32_t *offsets_host, const float *grad_enc, float *grad_inputs,
                                 uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                 uint32_t interpolation, int dtype, uint32_t grad_level_stride, void *stream) {
    if (D != 3 || C != 2 || interpolation != 0 || align_corners != 0 || gridtype > 1) return CNERF_EINVAL;
    if (dtype != CNERF_F32 && dtype != CNERF_F16) return CNERF_EINVAL;
    GridLevels lv;
    int rc = ge_levels(offsets_host, L, L, S, H, lv);
    if (rc) return rc;
    if (grad_level_stride == 0) grad_level_stride = B;
    if (grad_level_stride < B) return CNERF_EINVAL;
    if (B == 0) return CNERF_OK;
    if (!inputs || !embeddings || !grad_enc || !grad_inputs) return CNERF_ENULL;
    if (((uintptr_t)grad_enc) & 7) return CNERF_EINVAL;
    const dim3 grid(cn_div_up(B, FN_GIG_SAMPLES));
    if (dtype == CNERF_F16)
        hipLaunchKernelGGL(k_grid_input_grad<__half>, grid, dim3(GE_BLOCK), 0, CN_STREAM(stream), inputs, reinterpret_cast<const __half *>(embeddings), lv,
                           grad_enc, B, L, grad_level_stride, gridtype, grad_inputs);
    else
        hipLaunchKernelGGL(k_grid_input_grad<float>, grid, dim3(GE_BLOCK), 0, CN_STREAM(stream), inputs, reinterpret_cast<const float *>(embeddings), lv,
                           grad_enc, B, L, grad_level_stride, gridtype, grad_inputs);
    return cn_launch_status();
}

int cnerf_composite_normals(const float *weights, const int32_t *src_index, const float *grad_x, const float *dirs, uint32_t V, uint32_t N, uint32_t S,
                            uint32_t P_, float *normal_map, float *orient, void *stream) {
    if (V < 1 || V > FN_CN_VMAX || S == 0) return CNERF_EINVAL;
    if (N == 0) return CNERF_OK;
    if (!weights || !grad_x || !dirs || !normal_map || !orient) return CNERF_ENULL;
    if (!src_index && (uint64_t)N * S > P_) return CNERF_EINVAL;     // identity order: the sample list is the [N, S] block itself
    hipLaunchKernelGGL(k_composite_normals, dim3(cn_div_up(N, 4)), dim3(256), 0, CN_STREAM(stream), weights, src_index, grad_x, dirs, V, N, S, P_, normal_map,
                       orient);
    return cn_launch_status();
}

}  // extern "C"
