// Shared helpers for the gfx950 kernels.  Everything here is written for CDNA4 only (wave64, 256 CUs / 8 XCDs).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "../../include/customnerf_hip.h"

#define CN_WAVE 64
#define CN_NXCD 8

static inline int cn_launch_status() {
    hipError_t e = hipGetLastError();
    return (int)e;
}

static inline uint32_t cn_div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
static inline uint64_t cn_div_up64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

#define CN_STREAM(s) ((hipStream_t)(s))

// cnerf_profile_stage_events (misc.hip): event handles recorded between the kernels of a multi-kernel entry point; all NULL unless a benchmark set them
extern float *g_cn_found_inf;            // cnerf_scaler_watch (misc.hip): &state[2] of the watched loss scaler, or NULL
extern void *g_cn_stage_events[CNERF_STAGE_EVENTS];
static inline void cn_stage(int slot, hipStream_t st) {
    if (g_cn_stage_events[slot]) (void)hipEventRecord((hipEvent_t)g_cn_stage_events[slot], st);
}

// Measurement / tuning switches (kernel-generation selectors, sweep overrides, ablation masks) are read from the environment ONLY in builds
// made with `make TUNING=1` (-DCNERF_TUNING, used by the scratch/ scripts).  The release library always takes the default: nothing in the
// shipped .so changes behaviour with an environment variable.
#include <stdlib.h>
static inline int cn_tune_env(const char *name, int dflt) {
#ifdef CNERF_TUNING
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}
static inline double cn_tune_env_f(const char *name, double dflt) {
#ifdef CNERF_TUNING
    const char *e = getenv(name);
    return e ? atof(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// All float arithmetic in these kernels is compiled with -ffp-contract=off; fused multiply-adds are spelled out
// with cn_fma so that index-producing arithmetic is bit-identical to the oracle (oracle/raymarching_ref.c).
__device__ __forceinline__ float cn_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ float cn_clamp(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

// wave-level helpers (wave64)
__device__ __forceinline__ uint32_t cn_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// wave scans / sums on the DPP data path (row_shr inside the 16-lane rows, row_bcast:15 / :31 across them) — no ds_bpermute round trips
// in the per-ray dependency chains.  `old` is what a lane keeps when its DPP source lane does not exist or its row is masked (the identity).
#define CN_DPP_WAVE_SHR1 0x138                          // wave_shr:1: lane l reads lane l - 1
template <int CTRL, int ROW_MASK = 0xF, typename T>
__device__ __forceinline__ T cn_dpp(T old, T src) {
    static_assert(sizeof(T) == 4, "32-bit types only");
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK, typename T>
__device__ __forceinline__ T cn_dpp_zero(T src) { return cn_dpp<CTRL, ROW_MASK>(T(0), src); }

template <typename T>
__device__ __forceinline__ T cn_wave_incl_scan(T v) {   // inclusive prefix sum across the 64 lanes
    v += cn_dpp_zero<0x111, 0xF>(v);
    v += cn_dpp_zero<0x112, 0xF>(v);
    v += cn_dpp_zero<0x114, 0xF>(v);
    v += cn_dpp_zero<0x118, 0xF>(v);
    v += cn_dpp_zero<0x142, 0xA>(v);                     // row_bcast:15 into rows 1 and 3
    v += cn_dpp_zero<0x143, 0xC>(v);                     // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ float cn_wave_incl_prod(float x) {   // inclusive prefix product across the 64 lanes
    x *= cn_dpp<0x111>(1.0f, x);
    x *= cn_dpp<0x112>(1.0f, x);
    x *= cn_dpp<0x114>(1.0f, x);
    x *= cn_dpp<0x118>(1.0f, x);
    x *= cn_dpp<0x142, 0xA>(1.0f, x);
    x *= cn_dpp<0x143, 0xC>(1.0f, x);
    return x;
}

template <typename T>
__device__ __forceinline__ T cn_lane63(T v) {           // the last lane's value, wave-uniform
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
template <typename T>
__device__ __forceinline__ T cn_wave_sum(T v) { return cn_lane63(cn_wave_incl_scan(v)); }

// four floats -> four halves (round to nearest even) in one 8-byte value: the fp16 shadow of a parameter, the data-parallel payload
__device__ __forceinline__ uint2 cn_pack_half4(float4 f) {
    union { __half2 h[2]; uint2 u; } o;
    o.h[0] = __floats2half2_rn(f.x, f.y);
    o.h[1] = __floats2half2_rn(f.z, f.w);
    return o.u;
}

// near / far of a ray against an axis-aligned box (raymarching.cu:91-145): shared by k_near_far_from_aabb and the fused coarse sampler
#include <float.h>
__device__ __forceinline__ void cn_near_far(const float *__restrict__ o, const float *__restrict__ d, const float *__restrict__ aabb, float min_near,
                                            float &near_out, float &far_out) {
    const float ox = o[0], oy = o[1], oz = o[2];
    const float rdx = 1 / d[0], rdy = 1 / d[1], rdz = 1 / d[2];
    float near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx;
    if (near > far) { const float c = near; near = far; far = c; }
    float near_y = (aabb[1] - oy) * rdy, far_y = (aabb[4] - oy) * rdy;
    if (near_y > far_y) { const float c = near_y; near_y = far_y; far_y = c; }
    bool miss = (near > far_y || near_y > far);
    if (near_y > near) near = near_y;
    if (far_y < far) far = far_y;
    float near_z = (aabb[2] - oz) * rdz, far_z = (aabb[5] - oz) * rdz;
    if (near_z > far_z) { const float c = near_z; near_z = far_z; far_z = c; }
    miss = miss || (near > far_z || near_z > far);
    if (near_z > near) near = near_z;
    if (far_z < far) far = far_z;
    if (near < min_near) near = min_near;
    near_out = miss ? FLT_MAX : near;
    far_out = miss ? FLT_MAX : far;
}
