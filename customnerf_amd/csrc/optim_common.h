// The optimiser rules that several kernels apply and that have to give the same bits in each of them: the Adam element update and its
// bias correction (k_adam, k_adam_scaled, k_adam_scaled_multi in misc.hip; the table's step inside the scatter, gridencoder_binned.hip)
// and the GradScaler update (k_scaler_update, the last workgroup of k_adam_scaled_multi).  One definition each.
#pragma once
#include "common.h"
#include <math.h>

// torch.optim.Adam semantics (no weight decay, no amsgrad):  m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
// p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps), g being the stored gradient times gscale (the loss scale's inverse).
struct CnAdamK { float gscale, step_size, rsqrt_bc2, beta1, beta2, eps; };
__device__ __forceinline__ void cn_adam_elem(float &p, float &m, float &v, float g, const CnAdamK &k) {
    const float gk = g * k.gscale;
    m = k.beta1 * m + (1.0f - k.beta1) * gk;
    v = k.beta2 * v + (1.0f - k.beta2) * gk * gk;
    p -= k.step_size * m / (sqrtf(v) * k.rsqrt_bc2 + k.eps);
}

// bias correction of step `step` (1-based), in double precision as torch computes it on the host; each side uses its own libm.
// Three pieces, since k_adam_scaled_multi evaluates the powers once per workgroup and forms the step size per tensor from bc1.
__host__ __device__ __forceinline__ void cn_adam_bias(double step, float beta1, float beta2, double &bc1, double &bc2) {
    bc1 = 1.0 - pow((double)beta1, step);
    bc2 = 1.0 - pow((double)beta2, step);
}
__host__ __device__ __forceinline__ float cn_adam_step_size(float lr, double bc1) { return (float)((double)lr / bc1); }
__host__ __device__ __forceinline__ float cn_adam_rsqrt_bc2(double bc2) { return (float)(1.0 / sqrt(bc2)); }

// ---- the loss scaler's device state: float[4] {scale, growth_tracker, found_inf, good_steps}
// What an Adam step driven by the scaler takes from it.  Non-finite gradients in this step: optimizer.step() is skipped
__device__ __forceinline__ bool cn_scaler_skip(const float *state) { return state[2] != 0.0f; }
__device__ __forceinline__ float cn_scaler_gscale(const float *state, float extra_inv) { return extra_inv / state[0]; }
__device__ __forceinline__ double cn_scaler_step(const float *state) { return (double)state[3] + 1.0; }     // the step count is the good steps so far, plus this one
// torch.cuda.amp.GradScaler.update(); `skip` = cn_scaler_skip(state), read before any other workgroup could have cleared it
__device__ __forceinline__ void cn_scaler_update(float *state, bool skip, float growth, float backoff, float interval) {
    if (skip) { state[0] *= backoff; state[1] = 0.0f; }
    else {
        state[3] += 1.0f;
        const float t = state[1] + 1.0f;
        if (t >= interval) {
            const float grown = state[0] * growth;                        // torch keeps the old scale when the grown one would overflow,
            if (isfinite(grown)) state[0] = grown;                        // and resets the tracker either way
            state[1] = 0.0f;
        } else state[1] = t;
    }
    state[2] = 0.0f;
}
