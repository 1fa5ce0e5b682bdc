// Image comparison in one fused pass (cnerf_image_metrics, include/customnerf_hip.h): squared error, absolute error and the SSIM map of
// Wang et al. between two channel-last image batches, summed per image.  The reference scores nothing on the device (its evaluate loop
// hands numpy arrays to a PSNR meter, utils_init_nerf.py:673-779); the definition restated by tests/ssim_restatement.py is the header's.
//
// One workgroup per 32 x 32 output tile of one (image, channel).  The 42 x 42 input tile (the outputs' 11-tap footprint) of both images
// is staged in LDS once as float32 (float16 and float32 inputs convert exactly), the horizontal pass of the five window moments
// (a, b, aa, bb, ab) goes to LDS in float64, the vertical pass and the SSIM expression stay in registers, and a fixed-order workgroup
// reduction writes ONE partial (five doubles) per tile; k_image_metrics_sum adds an image's partials in a fixed order.  No atomics: the
// sums are bit-reproducible.  LDS: 2 x 42 x 42 x 4 + 5 x 42 x 32 x 8 = 67,872 bytes, two workgroups to a CU's 160 KiB.
//
// Why float64 moments: sigma = E[ab] - E[a]E[b] cancels and the quotient divides by as little as 9e-4.  In float32 a flat pair (1.0 against
// 0.9) loses 1.3e-4 of SSIM, flat + 1e-3 noise up to 2.8e-4 per window and a step edge 1.2e-4.  About 110 float64
// FMAs per pixel-channel is nothing beside the render that produced the pixel.
//
// cnerf_ssim_grad (the D-SSIM loss: metrics.ssim_loss, opt.lambda_dssim) is the same tile pass — one device routine,
// so the same sums bit for bit — that also stores three float64 coefficient maps per window, and k_ssim_grad_gather, which applies the
// transposed window to them per pixel: d ssim / d pred, float64 until one rounding to float32, no atomics either.
#include "common.h"

#define MT_TILE 32
#define MT_TAPS 11
#define MT_HALO (MT_TAPS - 1)
#define MT_IN (MT_TILE + MT_HALO)
#define MT_THREADS 256
#define MT_ROWS_PER_THREAD (MT_TILE * MT_TILE / MT_THREADS)          // 4 consecutive output rows of one column per thread
#define MT_NSUMS 5

struct MtWeights { double w[MT_TAPS]; };

// floor(clamp(v, 0, 1) * 255) / 255 in float32: what an 8-bit file of the image holds (the truncation of utils_init_nerf.py:550, plus a clamp)
__device__ __forceinline__ float mt_quantize(float v) { return floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f) / 255.0f; }

// sums of the workgroup's 256 per-thread values in a fixed (tree) order; s_red is [MT_NSUMS][MT_THREADS]; the result is valid on thread 0
__device__ __forceinline__ void mt_block_sums(double (&v)[MT_NSUMS], double *s_red) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int m = 0; m < MT_NSUMS; m++) s_red[m * MT_THREADS + t] = v[m];
    __syncthreads();
    for (uint32_t s = MT_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int m = 0; m < MT_NSUMS; m++) s_red[m * MT_THREADS + t] += s_red[m * MT_THREADS + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < MT_NSUMS; m++) v[m] = s_red[m * MT_THREADS];
}

// The tile pass both entry points share (k_image_metrics and k_ssim_maps are this routine and nothing else, so their partial sums are the same
// bits): error sums, window moments, the SSIM expression, one partial per tile.  COEF: also store the three coefficient maps of the gradient
// (cnerf_ssim_grad; the header has the formulas) at the tile's windows, as zeros where the window is not counted — coef is
// [B C][3][H - 10][W - 10] float64 in the order d_mu, d_aa, d_ab.
template <typename T, bool COEF>
__device__ __forceinline__ void mt_tile_pass(const T *__restrict__ pred, const T *__restrict__ target, const float *__restrict__ mask,
                                             uint32_t H, uint32_t W, uint32_t C, int quantize, const MtWeights &wt,
                                             double *__restrict__ partials, float *__restrict__ ssim_map, double *__restrict__ coef) {
    __shared__ float s_a[MT_IN][MT_IN], s_b[MT_IN][MT_IN];
    __shared__ double s_h[MT_NSUMS][MT_IN][MT_TILE];
    static_assert(sizeof(double) * MT_NSUMS * MT_IN * MT_TILE >= sizeof(double) * MT_NSUMS * MT_THREADS, "the reduction reuses s_h");
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.z / C, c = blockIdx.z - b * C;
    const uint32_t x0 = blockIdx.x * MT_TILE, y0 = blockIdx.y * MT_TILE;
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const uint32_t Hv = H - MT_HALO, Wv = W - MT_HALO;                  // the valid region of the map

    // stage both input tiles; every pixel of the image belongs to exactly one tile for the error sums: the tile whose 32 x 32 corner holds
    // it, and the last tile of a row / column takes the rest (at most 10 more, inside its halo: (n - 1) 32 + 32 >= extent - 10)
    double se = 0.0, ae = 0.0, npix = 0.0;
    for (uint32_t i = tid; i < MT_IN * MT_IN; i += MT_THREADS) {
        const uint32_t ly = i / MT_IN, lx = i - ly * MT_IN, y = y0 + ly, x = x0 + lx;
        float a = 0.0f, t = 0.0f;
        if (y < H && x < W) {
            const size_t p = ((size_t)b * H + y) * W + x;
            a = (float)pred[p * C + c];
            t = (float)target[p * C + c];
            if (quantize) { a = mt_quantize(a); t = mt_quantize(t); }
            if ((ly < MT_TILE || last_y) && (lx < MT_TILE || last_x) && (!mask || mask[p] != 0.0f)) {
                const double d = (double)a - (double)t;
                se += d * d;
                ae += fabs(d);
                npix += 1.0;
            }
        }
        s_a[ly][lx] = a;
        s_b[ly][lx] = t;
    }
    __syncthreads();

    // horizontal pass: five moments of every staged row at the tile's 32 columns
    for (uint32_t i = tid; i < MT_IN * MT_TILE; i += MT_THREADS) {
        const uint32_t r = i / MT_TILE, x = i - r * MT_TILE;
        double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
        for (int k = 0; k < MT_TAPS; k++) {
            const double a = (double)s_a[r][x + k], t = (double)s_b[r][x + k], w = wt.w[k];
            sa += w * a;
            sb += w * t;
            saa += w * (a * a);
            sbb += w * (t * t);
            sab += w * (a * t);
        }
        s_h[0][r][x] = sa; s_h[1][r][x] = sb; s_h[2][r][x] = saa; s_h[3][r][x] = sbb; s_h[4][r][x] = sab;
    }
    __syncthreads();

    // vertical pass in registers: one column, four consecutive output rows per thread (14 LDS reads per moment instead of 44)
    const uint32_t ox = tid % MT_TILE, oy0 = (tid / MT_TILE) * MT_ROWS_PER_THREAD;
    double mom[MT_NSUMS][MT_ROWS_PER_THREAD];
#pragma unroll
    for (int m = 0; m < MT_NSUMS; m++) {
        double v[MT_ROWS_PER_THREAD + MT_HALO];
#pragma unroll
        for (int j = 0; j < MT_ROWS_PER_THREAD + MT_HALO; j++) v[j] = s_h[m][oy0 + j][ox];
#pragma unroll
        for (int o = 0; o < MT_ROWS_PER_THREAD; o++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MT_TAPS; k++) s += wt.w[k] * v[o + k];
            mom[m][o] = s;
        }
    }
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;                   // (K1 L)^2, (K2 L)^2 with L = 1
    double ssum = 0.0, nwin = 0.0;
    const uint32_t x = x0 + ox;
#pragma unroll
    for (int o = 0; o < MT_ROWS_PER_THREAD; o++) {
        const uint32_t y = y0 + oy0 + o;
        if (y < Hv && x < Wv) {
            const double mu_a = mom[0][o], mu_b = mom[1][o];
            const double var_a = mom[2][o] - mu_a * mu_a, var_b = mom[3][o] - mu_b * mu_b, cov = mom[4][o] - mu_a * mu_b;
            const double A1 = 2.0 * (mu_a * mu_b) + C1, A2 = 2.0 * cov + C2, B1 = mu_a * mu_a + mu_b * mu_b + C1, B2 = var_a + var_b + C2;
            const double s = (A1 * A2) / (B1 * B2);
            if (ssim_map) ssim_map[(((size_t)b * Hv + y) * Wv + x) * C + c] = (float)s;
            const bool counted = !mask || mask[((size_t)b * H + y + MT_HALO / 2) * W + x + MT_HALO / 2] != 0.0f;   // a window counts by its centre pixel
            if (counted) {
                ssum += s;
                nwin += 1.0;
            }
            if (COEF) {
                const double r12 = 1.0 / (B1 * B2), r1 = 1.0 / B1, r2 = 1.0 / B2;
                const size_t plane = (size_t)Hv * Wv, at = (size_t)blockIdx.z * 3 * plane + (size_t)y * Wv + x;
                coef[at] = counted ? 2.0 * mu_b * (A2 - A1) * r12 + 2.0 * mu_a * s * (r2 - r1) : 0.0;
                coef[at + plane] = counted ? -s * r2 : 0.0;
                coef[at + 2 * plane] = counted ? 2.0 * A1 * r12 : 0.0;
            }
        }
    }
    __syncthreads();                                                    // everyone is done reading s_h: it becomes the reduction buffer
    double v[MT_NSUMS] = {se, ae, npix, ssum, nwin};
    mt_block_sums(v, &s_h[0][0][0]);
    if (tid == 0) {
        double *dst = partials + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * MT_NSUMS;
#pragma unroll
        for (int m = 0; m < MT_NSUMS; m++) dst[m] = v[m];
    }
}

template <typename T>
__global__ void __launch_bounds__(MT_THREADS) k_image_metrics(const T *__restrict__ pred, const T *__restrict__ target, const float *__restrict__ mask,
                                                              uint32_t H, uint32_t W, uint32_t C, int quantize, MtWeights wt,
                                                              double *__restrict__ partials, float *__restrict__ ssim_map) {
    mt_tile_pass<T, false>(pred, target, mask, H, W, C, quantize, wt, partials, ssim_map, nullptr);
}

// cnerf_ssim_grad, first launch: the same partials, plus the coefficient maps
template <typename T>
__global__ void __launch_bounds__(MT_THREADS) k_ssim_maps(const T *__restrict__ pred, const T *__restrict__ target, const float *__restrict__ mask,
                                                          uint32_t H, uint32_t W, uint32_t C, MtWeights wt, double *__restrict__ partials,
                                                          double *__restrict__ coef) {
    mt_tile_pass<T, true>(pred, target, mask, H, W, C, 0, wt, partials, nullptr, coef);
}

// sums_out[b][0..4] = the sum of image b's n partials: thread t adds partials t, t + 256, ... in that order, then the fixed tree
__global__ void __launch_bounds__(MT_THREADS) k_image_metrics_sum(const double *__restrict__ partials, uint32_t n, double *__restrict__ sums_out) {
    __shared__ double s_red[MT_NSUMS * MT_THREADS];
    const double *src = partials + (size_t)blockIdx.x * n * MT_NSUMS;
    double v[MT_NSUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n; i += MT_THREADS) {
#pragma unroll
        for (int m = 0; m < MT_NSUMS; m++) v[m] += src[(size_t)i * MT_NSUMS + m];
    }
    mt_block_sums(v, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int m = 0; m < MT_NSUMS; m++) sums_out[(size_t)blockIdx.x * MT_NSUMS + m] = v[m];
    }
}

// cnerf_ssim_grad, third launch: grad[q] = (T[d_mu](q) + 2 a(q) T[d_aa](q) + b(q) T[d_ab](q)) / n_windows, T the TRANSPOSED window filter
// T[m](y, x) = sum_k sum_l w[k] w[l] m(y - k, x - l), m zero outside the map.  A gather: one workgroup per 32 x 32 tile of PIXELS of one (image,
// channel) stages the 42 x 42 map footprint (windows y0 - 10 .. y0 + 31) of the three coefficient maps in LDS, filters rows into LDS and
// columns in registers, all float64, and rounds each element to float32 once.  No atomics: the same bits on every run.  n_windows is read
// from the reduced sums on the device; an image without a counted window gets exact zeros.
// LDS: 3 x 42 x 42 x 8 + 3 x 42 x 32 x 8 = 74,592 bytes, two workgroups to a CU's 160 KiB.
#define SG_NMAPS 3
template <typename T>
__global__ void __launch_bounds__(MT_THREADS) k_ssim_grad_gather(const T *__restrict__ pred, const T *__restrict__ target, const double *__restrict__ coef,
                                                                 const double *__restrict__ sums, uint32_t H, uint32_t W, uint32_t C, MtWeights wt,
                                                                 float *__restrict__ grad) {
    __shared__ double s_m[SG_NMAPS][MT_IN][MT_IN];
    __shared__ double s_h[SG_NMAPS][MT_IN][MT_TILE];
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.z / C, c = blockIdx.z - b * C;
    const uint32_t x0 = blockIdx.x * MT_TILE, y0 = blockIdx.y * MT_TILE;
    const uint32_t Hv = H - MT_HALO, Wv = W - MT_HALO;
    const uint32_t ox = tid % MT_TILE, oy0 = (tid / MT_TILE) * MT_ROWS_PER_THREAD;
    const double nwin = sums[(size_t)b * MT_NSUMS + 4];
    if (!(nwin > 0.0)) {                                                // (the same for the whole workgroup: nobody reaches a barrier)
#pragma unroll
        for (int o = 0; o < MT_ROWS_PER_THREAD; o++) {
            const uint32_t y = y0 + oy0 + o, x = x0 + ox;
            if (y < H && x < W) grad[(((size_t)b * H + y) * W + x) * C + c] = 0.0f;
        }
        return;
    }

    // stage the maps: local (ly, lx) is window (y0 + ly - 10, x0 + lx - 10), zero outside the valid region
    const size_t plane = (size_t)Hv * Wv;
    const double *src = coef + (size_t)blockIdx.z * SG_NMAPS * plane;
    for (uint32_t i = tid; i < MT_IN * MT_IN; i += MT_THREADS) {
        const uint32_t ly = i / MT_IN, lx = i - ly * MT_IN;
        const int64_t my = (int64_t)y0 + ly - MT_HALO, mx = (int64_t)x0 + lx - MT_HALO;
        const bool in = my >= 0 && my < (int64_t)Hv && mx >= 0 && mx < (int64_t)Wv;
        const size_t at = in ? (size_t)my * Wv + (size_t)mx : 0;
#pragma unroll
        for (int m = 0; m < SG_NMAPS; m++) s_m[m][ly][lx] = in ? src[m * plane + at] : 0.0;
    }
    __syncthreads();

    // rows: pixel column x0 + x takes window column x0 + x - l with weight w[l], i.e. local column x + k with w[10 - k]
    for (uint32_t i = tid; i < MT_IN * MT_TILE; i += MT_THREADS) {
        const uint32_t r = i / MT_TILE, x = i - r * MT_TILE;
#pragma unroll
        for (int m = 0; m < SG_NMAPS; m++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MT_TAPS; k++) s += wt.w[MT_HALO - k] * s_m[m][r][x + k];
            s_h[m][r][x] = s;
        }
    }
    __syncthreads();

    // columns in registers: one column, four consecutive pixel rows per thread
    double acc[SG_NMAPS][MT_ROWS_PER_THREAD];
#pragma unroll
    for (int m = 0; m < SG_NMAPS; m++) {
        double v[MT_ROWS_PER_THREAD + MT_HALO];
#pragma unroll
        for (int j = 0; j < MT_ROWS_PER_THREAD + MT_HALO; j++) v[j] = s_h[m][oy0 + j][ox];
#pragma unroll
        for (int o = 0; o < MT_ROWS_PER_THREAD; o++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MT_TAPS; k++) s += wt.w[MT_HALO - k] * v[o + k];
            acc[m][o] = s;
        }
    }
    const uint32_t x = x0 + ox;
#pragma unroll
    for (int o = 0; o < MT_ROWS_PER_THREAD; o++) {
        const uint32_t y = y0 + oy0 + o;
        if (y < H && x < W) {
            const size_t p = (((size_t)b * H + y) * W + x) * C + c;
            const double a = (double)(float)pred[p], t = (double)(float)target[p];
            grad[p] = (float)((acc[0][o] + 2.0 * a * acc[1][o] + t * acc[2][o]) / nwin);
        }
    }
}

// shapes both entry points accept: C in {1, 3}, H, W in [11, 65535], B C <= 65535 (the grid's z extent)
static bool mt_shape_ok(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    return (C == 1 || C == 3) && H >= MT_TAPS && W >= MT_TAPS && H <= 65535u && W <= 65535u && (uint64_t)B * C <= 65535u;
}
static uint32_t mt_tiles(uint32_t extent) { return cn_div_up(extent - MT_HALO, MT_TILE); }

// the 11-tap sigma 1.5 window, float64, normalised to sum 1
static MtWeights mt_window() {
    MtWeights wt;
    double total = 0.0;
    for (int k = 0; k < MT_TAPS; k++) {
        const double d = (double)(k - MT_TAPS / 2);
        wt.w[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        total += wt.w[k];
    }
    for (int k = 0; k < MT_TAPS; k++) wt.w[k] /= total;
    return wt;
}
static uint64_t mt_partial_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    return (uint64_t)B * C * mt_tiles(H) * mt_tiles(W) * MT_NSUMS * sizeof(double);
}

extern "C" {

int cnerf_image_metrics_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint64_t *bytes_host) {
    if (!mt_shape_ok(B, H, W, C)) return CNERF_EINVAL;
    if (!bytes_host) return CNERF_ENULL;
    *bytes_host = mt_partial_bytes(B, H, W, C);
    return CNERF_OK;
}

int cnerf_image_metrics(const void *pred, const void *target, const float *mask, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int dtype,
                        int quantize, double *sums_out, float *ssim_map, void *workspace, void *stream) {
    if (!mt_shape_ok(B, H, W, C) || (dtype != CNERF_F32 && dtype != CNERF_F16)) return CNERF_EINVAL;
    if (B == 0) return CNERF_OK;
    if (!pred || !target || !sums_out || !workspace) return CNERF_ENULL;
    if ((uintptr_t)workspace % sizeof(double) || (uintptr_t)sums_out % sizeof(double)) return CNERF_EINVAL;
    const MtWeights wt = mt_window();
    const dim3 grid(mt_tiles(W), mt_tiles(H), B * C);
    if (dtype == CNERF_F16)
        hipLaunchKernelGGL(k_image_metrics<_Float16>, grid, dim3(MT_THREADS), 0, CN_STREAM(stream), (const _Float16 *)pred, (const _Float16 *)target, mask,
                           H, W, C, quantize, wt, (double *)workspace, ssim_map);
    else
        hipLaunchKernelGGL(k_image_metrics<float>, grid, dim3(MT_THREADS), 0, CN_STREAM(stream), (const float *)pred, (const float *)target, mask,
                           H, W, C, quantize, wt, (double *)workspace, ssim_map);
    int rc = cn_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_image_metrics_sum, dim3(B), dim3(MT_THREADS), 0, CN_STREAM(stream), (const double *)workspace, C * grid.x * grid.y, sums_out);
    return cn_launch_status();
}

// workspace of cnerf_ssim_grad: the tile partials, then the three float64 coefficient maps [B C][3][H - 10][W - 10]
int cnerf_ssim_grad_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint64_t *bytes_host) {
    if (!mt_shape_ok(B, H, W, C)) return CNERF_EINVAL;
    if (!bytes_host) return CNERF_ENULL;
    *bytes_host = mt_partial_bytes(B, H, W, C) + (uint64_t)B * C * SG_NMAPS * (H - MT_HALO) * (W - MT_HALO) * sizeof(double);
    return CNERF_OK;
}

int cnerf_ssim_grad(const void *pred, const void *target, const float *mask, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int dtype,
                    double *sums_out, float *grad_unit, void *workspace, void *stream) {
    if (!mt_shape_ok(B, H, W, C) || (dtype != CNERF_F32 && dtype != CNERF_F16)) return CNERF_EINVAL;
    if (B == 0) return CNERF_OK;
    if (!pred || !target || !sums_out || !grad_unit || !workspace) return CNERF_ENULL;
    if ((uintptr_t)workspace % sizeof(double) || (uintptr_t)sums_out % sizeof(double) || (uintptr_t)grad_unit % sizeof(float)) return CNERF_EINVAL;
    const MtWeights wt = mt_window();
    double *partials = (double *)workspace;
    double *coef = partials + mt_partial_bytes(B, H, W, C) / sizeof(double);
    const dim3 grid(mt_tiles(W), mt_tiles(H), B * C), pixels(cn_div_up(W, MT_TILE), cn_div_up(H, MT_TILE), B * C);
    if (dtype == CNERF_F16)
        hipLaunchKernelGGL(k_ssim_maps<_Float16>, grid, dim3(MT_THREADS), 0, CN_STREAM(stream), (const _Float16 *)pred, (const _Float16 *)target, mask,
                           H, W, C, wt, partials, coef);
    else
        hipLaunchKernelGGL(k_ssim_maps<float>, grid, dim3(MT_THREADS), 0, CN_STREAM(stream), (const float *)pred, (const float *)target, mask,
                           H, W, C, wt, partials, coef);
    int rc = cn_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(k_image_metrics_sum, dim3(B), dim3(MT_THREADS), 0, CN_STREAM(stream), (const double *)partials, C * grid.x * grid.y, sums_out);
    rc = cn_launch_status();
    if (rc) return rc;
    if (dtype == CNERF_F16)
        hipLaunchKernelGGL(k_ssim_grad_gather<_Float16>, pixels, dim3(MT_THREADS), 0, CN_STREAM(stream), (const _Float16 *)pred, (const _Float16 *)target,
                           (const double *)coef, (const double *)sums_out, H, W, C, wt, grad_unit);
    else
        hipLaunchKernelGGL(k_ssim_grad_gather<float>, pixels, dim3(MT_THREADS), 0, CN_STREAM(stream), (const float *)pred, (const float *)target,
                           (const double *)coef, (const double *)sums_out, H, W, C, wt, grad_unit);
    return cn_launch_status();
}

}  // extern "C"
