// Image sampling glue of the SD half: what sits between the UNet / the VAE decoder and the float32 latents of a DDIM run
// (StableDiffusion.produce_latents / decode_latents / preview).  Each entry point is one launch on the caller's stream; all three
// are latency-bound element-wise passes (a 64 x 64 latent is 4096 pixels), float32 arithmetic, one thread per pixel.
#include "common.h"
#include "../../include/customnerf_sd.h"

#define SS_THREADS 256
typedef _Float16 ss_h8 __attribute__((ext_vector_type(8)));
static inline uint32_t ss_blocks(size_t n) { return (uint32_t)((n + SS_THREADS - 1) / SS_THREADS); }

// ------------------------------------------------------------------------------------------------ latents -> decoder input
// latents [B][4][hw] float32 -> [B][hw][8] half = post_quant_conv(latents / scaling_factor) (a 4 x 4 matrix and its bias: wb = W[out][in]
// row-major, then b[4]), channels 4..7 zero: the operand layout of decoder.conv_in (pack.pack_conv pads Cin to 8)
__global__ void __launch_bounds__(SS_THREADS) k_decoder_input(const float *__restrict__ latents, uint32_t B, uint32_t hw, float sf, const float *__restrict__ wb,
                                                              _Float16 *__restrict__ out) {
    const uint32_t i = blockIdx.x * SS_THREADS + threadIdx.x;                     // one pixel of one image
    if (i >= B * hw) return;
    const uint32_t b = i / hw, p = i - b * hw;
    // float64: z is ~5x the latents and the four products may cancel — a float32 sum is then off by more than a half ulp of the small
    // result.  Twenty multiply-adds per pixel on the full-rate FP64 units: not what this launch spends its time on.
    double z[4];
#pragma unroll
    for (int c = 0; c < 4; c++) z[c] = (double)latents[((size_t)b * 4 + c) * hw + p] / (double)sf;
    ss_h8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < 4; n++) {
        double acc = (double)wb[16 + n];
#pragma unroll
        for (int c = 0; c < 4; c++) acc += (double)wb[n * 4 + c] * z[c];
        o[n] = (_Float16)(float)acc;
    }
    *reinterpret_cast<ss_h8 *>(out + (size_t)i * 8) = o;
}

// ------------------------------------------------------------------------------------------------ decoder output -> images
// x [B][HW][ld] half (decoder.conv_out, channels 0..2) -> img [B][3][HW] float32 = clamp(x / 2 + 0.5, 0, 1) and, when asked for,
// img_u8 [B][HW][3] = round(255 img) (round half to even, like torch.round)
__global__ void __launch_bounds__(SS_THREADS) k_decoder_output(const _Float16 *__restrict__ x, uint32_t ld, uint32_t B, uint32_t HW, float *__restrict__ img,
                                                               uint8_t *__restrict__ img_u8) {
    const size_t i = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const size_t b = i / HW, p = i - b * HW;
    const _Float16 *src = x + i * ld;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float v = fminf(fmaxf((float)src[c] * 0.5f + 0.5f, 0.0f), 1.0f);
        if (img) img[(b * 3 + c) * HW + p] = v;
        if (img_u8) img_u8[i * 3 + c] = (uint8_t)rintf(255.0f * v);
    }
}

// ------------------------------------------------------------------------------------------------ one DDIM step (eta = 0)
// eps [pairs][2][pixels][ld] half (uncond, text); x [pairs][4][pixels] float32.  MODE 0: e = e_u + g (e_t - e_u) (classifier-free
// guidance); MODE 1: e = e_t + g (e_t - e_u) (the combination the SDS gradient uses: cnerf_sd_sds_grad).
//   x0 = (x - sqrt(1 - ab_t) e) / sqrt(ab_t);   x_prev = sqrt(ab_prev) x0 + sqrt(1 - ab_prev) e
// Outputs (each may be NULL): x_prev and x0 in x's layout (x_prev may be x itself: a thread reads its pixel before it writes it), and the
// next UNet input [pairs][2][pixels][8] half = x_prev twice, channels 4..7 zero (cnerf_sd_add_noise's layout).
__global__ void __launch_bounds__(SS_THREADS) k_ddim_step(const _Float16 *__restrict__ eps, uint32_t ld, const float *x, float sa_t, float sb_t, float sa_p,
                                                          float sb_p, float g, int mode, uint32_t pairs, uint32_t pixels, float *x_prev, float *__restrict__ x0_out,
                                                          _Float16 *__restrict__ unet_in) {
    const uint32_t i = blockIdx.x * SS_THREADS + threadIdx.x;
    if (i >= pairs * pixels) return;
    const uint32_t b = i / pixels, p = i - b * pixels;
    const _Float16 *eu = eps + ((size_t)(2 * b) * pixels + p) * ld, *et = eu + (size_t)pixels * ld;
    ss_h8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const size_t j = ((size_t)b * 4 + c) * pixels + p;
        const float u = (float)eu[c], t = (float)et[c];
        const float e = (mode == 0 ? u : t) + g * (t - u);
        const float x0 = (x[j] - sb_t * e) / sa_t;
        const float xp = sa_p * x0 + sb_p * e;
        if (x_prev) x_prev[j] = xp;
        if (x0_out) x0_out[j] = x0;
        o[c] = (_Float16)xp;
    }
    if (unet_in) {
        _Float16 *dst = unet_in + ((size_t)(2 * b) * pixels + p) * 8;
        *reinterpret_cast<ss_h8 *>(dst) = o;
        *reinterpret_cast<ss_h8 *>(dst + (size_t)pixels * 8) = o;
    }
}

// ================================================================================================ C ABI
int cnerf_sd_decoder_input(const float *latents, uint32_t B, uint32_t hw, float scaling_factor, const float *post_quant, void *out, void *stream) {
    if (!latents || !post_quant || !out) return CNERF_EINVAL;
    if (B == 0 || hw == 0 || (uint64_t)B * hw * 8 >= (1ull << 31) || !(scaling_factor > 0.0f) || (((uintptr_t)out) & 15)) return CNERF_EINVAL;
    hipLaunchKernelGGL(k_decoder_input, dim3(ss_blocks((size_t)B * hw)), dim3(SS_THREADS), 0, CN_STREAM(stream), latents, B, hw, scaling_factor, post_quant,
                       (_Float16 *)out);
    return cn_launch_status();
}

int cnerf_sd_decoder_output(const void *x, uint32_t ld, uint32_t B, uint32_t HW, float *img, uint8_t *img_u8, void *stream) {
    if (!x || (!img && !img_u8)) return CNERF_EINVAL;
    if (B == 0 || HW == 0 || ld < 3 || (uint64_t)B * HW >= (1ull << 31)) return CNERF_EINVAL;
    hipLaunchKernelGGL(k_decoder_output, dim3(ss_blocks((size_t)B * HW)), dim3(SS_THREADS), 0, CN_STREAM(stream), (const _Float16 *)x, ld, B, HW, img, img_u8);
    return cn_launch_status();
}

int cnerf_sd_ddim_step(const void *eps, uint32_t ld_eps, const float *latents, float alpha_bar_t, float alpha_bar_prev, float guidance, int mode, uint32_t pairs,
                       uint32_t pixels, float *latents_out, float *x0_out, void *unet_in, void *stream) {
    if (!eps || !latents || (!latents_out && !x0_out && !unet_in)) return CNERF_EINVAL;
    if (pairs == 0 || pixels == 0 || ld_eps < 4 || (uint64_t)pairs * pixels * 16 >= (1ull << 31) || (mode != 0 && mode != 1)) return CNERF_EINVAL;
    if (!(alpha_bar_t > 0.0f && alpha_bar_t <= 1.0f) || !(alpha_bar_prev > 0.0f && alpha_bar_prev <= 1.0f)) return CNERF_EINVAL;
    if (((uintptr_t)unet_in) & 15) return CNERF_EINVAL;
    const float sa_t = (float)sqrt((double)alpha_bar_t), sb_t = (float)sqrt(1.0 - (double)alpha_bar_t);
    const float sa_p = (float)sqrt((double)alpha_bar_prev), sb_p = (float)sqrt(1.0 - (double)alpha_bar_prev);
    hipLaunchKernelGGL(k_ddim_step, dim3(ss_blocks((size_t)pairs * pixels)), dim3(SS_THREADS), 0, CN_STREAM(stream), (const _Float16 *)eps, ld_eps, latents, sa_t,
                       sb_t, sa_p, sb_p, guidance, mode, pairs, pixels, latents_out, x0_out, (_Float16 *)unet_in);
    return cn_launch_status();
}
