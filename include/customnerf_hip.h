/*
 * customnerf_hip.h — C-ABI of libcustomnerf_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for CustomNeRF's volumetric-rendering hot path.  Each entry point replaces one function of
 * the reference's two native torch extensions (pybind modules `_raymarching`, `_gridencoder`) or one
 * third-party call on the path (tinycudann FullyFusedMLP).  Reference interfaces are cited per function as
 * file:line under /root/reference.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types.  Pointers are DEVICE pointers unless the name ends in `_host`.
 *   - caller owns every buffer; nothing is allocated, nothing synchronises with the host; work is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = the null stream).
 *   - returns 0 on success, a positive hipError_t if a launch failed, or a negative CNERF_E* code for rejected
 *     arguments (the reference raises std::runtime_error / TORCH_CHECK there: gridencoder.cu:380,397,448-464).
 *   - float32 data unless stated; `dtype` 0 = float32, 1 = float16 (IEEE binary16).
 */
#ifndef CUSTOMNERF_HIP_H
#define CUSTOMNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNERF_OK 0
#define CNERF_EINVAL (-1)      /* unsupported D / C / dtype / size */
#define CNERF_ENULL (-2)       /* required pointer is NULL */

#define CNERF_F32 0
#define CNERF_F16 1

/* ABI version of this header; cnerf_abi_version() of the loaded library must match.
 * 2: the GroupNorm / GEMM-epilogue statistics buffers of customnerf_sd.h are int64[B][G][2] fixed point (were float[B][G][2]).
 * 4: struct CnerfSdGemm grew the ln_* fields (LayerNorm of the output rows in the split-K tail); new entry points
 *    cnerf_grid_encode_forward_ordered, cnerf_sd_concat_gn, cnerf_sd_gemm_serves_ln, cnerf_profile_stage_events.
 * 6: the plan in pieces is gone — the _block / _rows / _finish variants of cnerf_grid_encode_backward_prepare (no shape took them since ABI 5).
 * 7: mesh extraction — cnerf_marching_cubes_workspace_bytes / _count / _emit; mesh cleanup (additive, same version: a binding that
 *    needs them fails at load on the missing symbol) — cnerf_mesh_components_* and cnerf_mesh_cluster_* (workspace_bytes / _count / _emit);
 *    quadric decimation (additive, same version) — cnerf_mesh_decimate_workspace_bytes / _init / _round / _emit; texture baking (additive,
 *    same version) — cnerf_mesh_atlas_layout / _uvs / _points / _store / _fill; smoothing and normals (additive, same version) —
 *    cnerf_mesh_smooth_workspace_bytes / _init / _steps / _normals; mesh rasteriser (additive, same version) —
 *    cnerf_mesh_raster_workspace_bytes / _visibility / _shade; closest-point queries and surface samples (additive, same version) —
 *    cnerf_mesh_bvh_workspace_bytes / _build / _closest and cnerf_mesh_sample_workspace_bytes / _count / _emit; ray queries on the same tree
 *    (additive, same version) — cnerf_mesh_bvh_raycast / _occluded; the area-proportional atlas (additive, same version) —
 *    cnerf_mesh_atlas_sized_workspace_bytes / _measure / _layout / _plan / _uvs / _points / _store / _fill; projection onto a source
 *    mesh (additive, same version) — cnerf_mesh_bvh_project; the chart-based atlas (additive, same version) —
 *    cnerf_mesh_atlas_proj_workspace_bytes / _charts / _pack / _raster / _points / _store / _fill; welded vertices, tangent frames and
 *    tangent-space normal maps (additive, same version) — cnerf_mesh_tangent_workspace_bytes / _weld / _frames / _vertices and
 *    cnerf_mesh_atlas_tspace / cnerf_mesh_atlas_sized_tspace / cnerf_mesh_atlas_proj_tspace; marching cubes over a list of bricks
 *    (additive, same version) — cnerf_marching_cubes_sparse_workspace_bytes / _count / _emit; TSDF fusion of depth maps (additive, same
 *    version) — cnerf_tsdf_integrate / _finalize / _face_keep; topology report and hole filling (additive, same version) —
 *    cnerf_mesh_holes_workspace_bytes / _count / _emit and cnerf_mesh_topology / _loops; winding number and signed distance on the
 *    closest-point tree (additive, same version) — cnerf_mesh_winding_workspace_bytes / _build / _query and
 *    cnerf_mesh_bvh_signed_distance.
 * 8: the scatter's ahead-of-time plan is gone — cnerf_grid_encode_backward_prepare / _needs_plan / _prepared (cnerf_grid_encode_backward is
 *    the one call, on one stream) — and so is cnerf_grid_encode_forward_strided (cnerf_grid_encode_forward_ordered with CNERF_GRID_LEVEL_MAJOR).
 *    Ray regularisers (additive, same version) — cnerf_ray_reg_forward / cnerf_ray_reg_backward. */
#define CNERF_ABI_VERSION 8
int cnerf_abi_version(void);
/* name of the code object's target ("gfx950") */
const char *cnerf_target_arch(void);
/* Measurement aid (bench.py `variants.small_batch`; no reference counterpart): hipEvent_t handles that the multi-kernel entry points record on
 * their launch stream between their kernels, or NULL entries / n = 0 to switch it off (the default).  Slots:
 *   0 / 1 before / after the scatter's emit kernel, 2 after its accumulate kernel, 3 after its split-bin reduction (cnerf_grid_encode_backward*);
 *   4 / 5 before / after the field backward's main kernel, 6 after its partial-gradient reduction (cnerf_field_backward*).
 * The handles are borrowed: the caller keeps them alive until it clears the slots. */
#define CNERF_STAGE_EVENTS 8
int cnerf_profile_stage_events(void *const *events, uint32_t n);

/* ------------------------------------------------------------------------------------------------
 * _raymarching  (reference: raymarching/src/raymarching.h:7-21, bindings.cpp:5-20)
 * ---------------------------------------------------------------------------------------------- */

/* near_far_from_aabb — raymarching.h:7, kernel raymarching.cu:91-145.
 * rays_o, rays_d [N,3]; aabb [6]; nears, fars [N] (miss: both = FLT_MAX). */
int cnerf_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N,
                             float min_near, float *nears, float *fars, void *stream);

/* sph_from_ray — raymarching.h:8, kernel raymarching.cu:162-198.  coords [N,2]. */
int cnerf_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N, float *coords, void *stream);

/* morton3D / morton3D_invert — raymarching.h:9-10, kernels raymarching.cu:214-226, 237-254. */
int cnerf_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, void *stream);
int cnerf_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, void *stream);

/* packbits — raymarching.h:11, kernel raymarching.cu:267-289.  grid [N*8] floats -> bitfield [N] bytes. */
int cnerf_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, void *stream);

/* Occupancy-grid refresh — NeRFRenderer.update_extra_state (nerf/renderer.py:1658-1715) without its Python loops, temporary grid and
 * host synchronisations.  Per cascade: cnerf_occupancy_points -> the caller's density query -> cnerf_occupancy_update; then once
 * cnerf_occupancy_finalize_pack.
 *   points:   rand [H^3, 3] U[0,1) (the `torch.rand_like` draw of :1695) -> xyzs [H^3, 3], cell i = (x, y, z) in meshgrid('ij') order
 *             (:1679-1684): xyzs = (2 c / (H-1) - 1) * (cas_bound - half_grid) + (2 rand - 1) * half_grid  (:1690-1695);
 *   update:   sigmas [H^3] in the same order; density_grid_cascade [H^3] (Morton order, :1688 + :1697) gets max(old * decay, sigma) where
 *             old >= 0 (:1707-1709); partials [ceil(H^3 / 256)][2] doubles receive (sum, count) of the valid cells of this cascade;
 *   finalize: partials of ALL cascades [n_partials][2] -> state[0] = mean density of the valid cells (:1710), state[1] = min(mean,
 *             density_thresh) (:1712); bitfield [n_bytes] = packbits(density_grid [n_bytes * 8], state[1]) (:1713, raymarching.cu:267-289). */
int cnerf_occupancy_points(const float *rand, uint32_t H, float cas_bound, float half_grid, float *xyzs, void *stream);
int cnerf_occupancy_update(const float *sigmas, uint32_t H, float decay, float *density_grid_cascade, double *partials, void *stream);
int cnerf_occupancy_finalize_pack(const double *partials, uint32_t n_partials, float density_thresh, const float *density_grid,
                                  uint32_t n_bytes, float *state, uint8_t *bitfield, void *stream);

/* march_rays_train — raymarching.h:13, kernel raymarching.cu:311-480.
 * Same arguments as the reference binding.  Unlike the reference (atomics-ordered, nondeterministic slots) the
 * sample segments are laid out in RAY ORDER by an exclusive scan: rays[n] = (n, offset_n, num_steps_n).
 * counter[0] += total samples, counter[1] += N.  Rays with offset+num_steps > M are dropped (as :416); a call that overflows its
 * budget (counter[0] + total > M) starts the scan at ray floor(noises[0] * N) and wraps, so that the dropped rays move with the
 * per-call jitter draw instead of always being the highest-numbered ones (the reference drops in atomics arrival order).
 * xyzs/dirs [M,3], deltas [M,2], rays [N,3] int32, counter [2] int32, noises [N]. */
int cnerf_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                           uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                           const float *fars, float *xyzs, float *dirs, float *deltas, int32_t *rays, int32_t *counter,
                           const float *noises, void *stream);
/* The same operation split in its two passes so a caller can size xyzs/dirs/deltas from counter[0] instead of
 * pre-allocating N*max_steps samples (raymarching.py:197,206-208): _count fills rays[] and counter[];
 * _write (given the rays[] produced by _count) writes the samples. */
int cnerf_march_rays_train_count(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                                 uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, const float *nears,
                                 const float *fars, int32_t *rays, int32_t *counter, const float *noises, void *stream);
int cnerf_march_rays_train_write(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                                 uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears,
                                 const float *fars, float *xyzs, float *dirs, float *deltas, const int32_t *rays,
                                 const float *noises, void *stream);
/* The two passes without the second march: _count_hits additionally records (t, dt) of every occupied probe of ray n at
 * hits[n][step] (hits float32 [N, max_steps, 2], 8-byte aligned, caller-owned scratch; only the first num_steps_n entries of a row are
 * written); _write_hits turns the list into xyzs / dirs / deltas — one wave per ray, no occupancy lookups — with the arithmetic of
 * _write, bit for bit. */
int cnerf_march_rays_train_count_hits(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                                      uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, const float *nears,
                                      const float *fars, int32_t *rays, int32_t *counter, const float *noises, float *hits,
                                      void *stream);
int cnerf_march_rays_train_write_hits(const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                      uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float *nears, const float *noises,
                                      const float *hits, const int32_t *rays, float *xyzs, float *dirs, float *deltas,
                                      void *stream);

/* composite_rays_train_forward / _backward — raymarching.h:14-15 (the `_sdf` twins :16-17 are byte-identical
 * duplicates in the reference and map to the same entry points); kernels raymarching.cu:500-577, 691-772.
 * rgbs has `rgb_stride` floats per sample (3 in the reference binding; 4 lets a caller pass the field's
 * rgb+confidence rows without a slice/copy — renderer.py:630-635 passes such a tensor). */
int cnerf_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                                       uint32_t M, uint32_t N, float T_thresh, float *weights_sum, float *depth,
                                       float *image, uint32_t rgb_stride, void *stream);
int cnerf_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image, const float *sigmas,
                                        const float *rgbs, const float *deltas, const int32_t *rays,
                                        const float *weights_sum, const float *image, uint32_t M, uint32_t N,
                                        float T_thresh, float *grad_sigmas, float *grad_rgbs, uint32_t rgb_stride,
                                        void *stream);

/* march_rays / composite_rays (inference) — raymarching.h:19-20, kernels raymarching.cu:884-989, 1002-1089. */
int cnerf_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                     const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                     uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, float *xyzs,
                     float *dirs, float *deltas, const float *noises, void *stream);
int cnerf_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                         const float *sigmas, const float *rgbs, const float *deltas, float *weights_sum, float *depth,
                         float *image, uint32_t rgb_stride, void *stream);
/* Order-preserving device-side compaction replacing `rays_alive = rays_alive[rays_alive >= 0]`
 * (renderer.py:685): out[0..count) = the non-negative entries of in[0..n) in order, *count = their number.
 * Wave ballot + prefix scan; `count` is a device int32. */
int cnerf_compact_rays_alive(const int32_t *rays_alive_in, uint32_t n, int32_t *rays_alive_out, int32_t *count, void *stream);

/* ------------------------------------------------------------------------------------------------
 * _gridencoder  (reference: gridencoder/src/gridencoder.h:12-15, bindings.cpp:5-7)
 * ---------------------------------------------------------------------------------------------- */

/* grid_encode_forward — gridencoder.h:12, kernel gridencoder.cu:87-244.
 * inputs [B,D] in [0,1]; embeddings [offsets[L], C] (dtype); outputs [L,B,C] (dtype); dy_dx [B, L*D*C] (dtype) or NULL.
 * offsets_host: HOST int32 [L+1] (the reference passes a device tensor; the level geometry — scale, resolution,
 * table size — is derived from it on the host and travels as kernel arguments).
 * S = log2(per_level_scale), H = base resolution.  gridtype 0 hash / 1 tiled; interp 0 linear / 1 smoothstep.
 * D in {2,3,4,5}, C in {1,2,4,8}, L <= 32 — else CNERF_EINVAL (gridencoder.cu:380,397). */
int cnerf_grid_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets_host, void *outputs,
                              uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level, float S, uint32_t H,
                              void *dy_dx, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, void *stream);
/* Same, writing into a larger output buffer: outputs [L, out_level_stride, C] with out_level_stride >= B rows per level (0 = B);
 * the caller offsets `outputs` to the first row it wants written.  Lets several gathers (the coarse and the importance samples of
 * NeRFRenderer.run, renderer.py:327-363) fill one feature buffer, so that the coarse samples are not gathered a second time. */
/* ... and with the traversal of the sample list chosen by the caller (results are bit-identical either way; only the specialised
 * fp16 / D = 3 / C = 2 / linear kernel has two forms, every other configuration ignores it):
 *   CNERF_GRID_LEVEL_MAJOR  0  one level at a time per XCD (its table stays in that XCD's L2): right for samples spread over the volume
 *                              — the stratified samples of NeRFRenderer.run (renderer.py:317-325) — and what cnerf_grid_encode_forward takes;
 *   CNERF_GRID_SAMPLE_MAJOR 1  all levels of a tile of consecutive samples per workgroup: right when neighbours of the list are neighbours
 *                              in space — the importance samples (renderer.py:340-352) of a field that has a surface. */
#define CNERF_GRID_LEVEL_MAJOR 0
#define CNERF_GRID_SAMPLE_MAJOR 1
int cnerf_grid_encode_forward_ordered(const float *inputs, const void *embeddings, const int32_t *offsets_host, void *outputs,
                                      uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level, float S, uint32_t H,
                                      void *dy_dx, uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                      uint32_t out_level_stride, uint32_t traversal, void *stream);

/* grid_encode_backward — gridencoder.h:13, kernels gridencoder.cu:247-339 (+ :342-368 when dy_dx != NULL).
 * grad [L,B,C] (dtype).  grad_embeddings is ALWAYS float32 [offsets[L], C], pre-zeroed by the caller
 * (grid.py:83) and accumulated with float32 atomics (the reference uses __half2 atomics for fp16 tables).
 * grad_inputs float32 [B,D] (written, not accumulated) when dy_dx != NULL.
 * workspace (optional, 256-byte aligned device scratch of at least cnerf_grid_encode_backward_workspace_bytes()):
 * when given, large D=3/C=2 scatters run the atomic-free binned path (records partitioned by 4096-entry table
 * chunk, summed in LDS — exact 64-bit fixed point for fp16 tables, hence bit-reproducible — and added to grad_embeddings
 * with plain coalesced read-modify-writes); with NULL, or for other shapes / small B, the scatter uses global float
 * atomics.  Both produce the same sums up to float reassociation (fp16: up to the rounding of each w*g product). */
int cnerf_grid_encode_backward(const void *grad, const float *inputs, const int32_t *offsets_host, float *grad_embeddings,
                               uint32_t B, uint32_t D, uint32_t C, uint32_t L, uint32_t max_level, float S, uint32_t H,
                               const void *dy_dx, float *grad_inputs, uint32_t gridtype, int align_corners,
                               uint32_t interp, int dtype, void *workspace, uint64_t workspace_bytes, void *stream);
/* *bytes = scratch size the binned scatter wants for this problem (0: the atomic path will be used). */
int cnerf_grid_encode_backward_workspace_bytes(const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                               uint32_t max_level, float S, uint32_t H, int dtype, uint64_t *bytes);

/* grad_total_variation — gridencoder.h:15, kernel gridencoder.cu:505-609.  float32 only (grid.py:171). */
int cnerf_grad_total_variation(const float *inputs, const float *embeddings, float *grad, const int32_t *offsets_host,
                               float weight, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                               uint32_t gridtype, int align_corners, void *stream);

/* float32 -> float16 shadow copy of a table (what `embeddings.to(torch.half)` does under autocast, grid.py:45-46). */
int cnerf_cast_f32_to_f16(const float *src, void *dst, uint64_t n, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fused field evaluation: NeRFNetwork.forward / .density (nerf/network_grid.py:159-193) in one launch on the matrix
 * cores — the tinycudann FullyFusedMLP x3 of the reference (network_grid.py:98-139) plus its glue:
 *   fea   = MLP_net(enc)                                 enc_dim -> 64 x n_hidden_geo -> 64   (no output activation)
 *   sigma = exp(MLP_den(fea)[0] + 5 exp(-|x|^2 / 0.08))  64 -> 64 -> 1   (trunc_exp fwd provider_utils.py:20-22; blob :150-156)
 *   rgbc  = sigmoid(MLP_rgb([freq(d) (27), fea (64)]))   91 -> 64 -> n_rgb_out (3, or 4 = rgb + confidence; base.py:42-60)
 * MLPs are bias-free, ReLU hidden; params_* are the float32 flat vectors of tcnn.Network (row-major [out,in] matrices,
 * in padded to x16, out padded to x16: 64*pad16(enc_dim) + 4096*n_hidden_geo, 5120, 7168 floats).
 * enc is the grid encoder output in ITS kernel layout [L, P, 2] (dtype), so no permute copy is needed (grid.py:49,63).
 * xyz [P,3]; dirs [ceil(P/dir_group), 3]: one direction per dir_group consecutive samples (1 = per sample).
 * sigma float32 [P]; rgbc float32 [P,4] 16-byte aligned (NULL => density only; channel 3 is 0 when n_rgb_out == 3).
 * dtype CNERF_F16: fp16 weights/activations, fp32 accumulate (v_mfma_f32_32x32x16_f16), outputs rounded to fp16 values
 * — tcnn's numerics; CNERF_F32: exact float32 (v_mfma_f32_32x32x2_f32).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_field_forward(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                        uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                        const float *params_rgb, float *sigma, float *rgbc, int dtype, void *stream);
/* Same, reading the first P samples of an enc buffer that holds enc_level_stride >= P samples per level (0 = P). */
int cnerf_field_forward_strided(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                                uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                                const float *params_rgb, float *sigma, float *rgbc, int dtype, uint32_t enc_level_stride,
                                void *stream);

/* Backward of cnerf_field_forward (activations are recomputed, nothing is saved by the forward).
 * grad_sigma [P] and grad_rgbc [P,4] (16-byte aligned) in; grad_enc [L,P,2] (dtype) out = d(loss)/d(grid features) in the
 * encoder's kernel layout (feeds cnerf_grid_encode_backward directly); grad_params_* float32, ACCUMULATED (caller
 * pre-zeroes).  trunc_exp backward clamps the exponent to [-15,15] (provider_utils.py:26-29); positions and directions
 * receive no gradient on this path.  workspace: 16-byte aligned scratch of cnerf_field_backward_workspace_bytes(). */
int cnerf_field_backward(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                         uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                         const float *params_rgb, const float *grad_sigma, const float *grad_rgbc, void *grad_enc,
                         float *grad_params_net, float *grad_params_den, float *grad_params_rgb, void *workspace,
                         uint64_t workspace_bytes, int dtype, void *stream);
/* cnerf_field_backward with early termination: tile_live (optional) = the uint8 [ceil(P / 32)] flags of
 * cnerf_composite_run_backward_indexed_flush — a zero byte promises that grad_sigma / grad_rgbc of rows 32 k .. 32 k + 31 are exactly zero; the
 * kernel then skips the tile (its rows of grad_enc are written as zeros, the weight gradients are bit-identical: skipped tiles add exact zeros). */
int cnerf_field_backward_ex(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                            uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                            const float *params_rgb, const float *grad_sigma, const float *grad_rgbc, void *grad_enc,
                            float *grad_params_net, float *grad_params_den, float *grad_params_rgb, void *workspace,
                            uint64_t workspace_bytes, int dtype, const uint8_t *tile_live, void *stream);
int cnerf_field_backward_workspace_bytes(uint32_t P, uint32_t enc_dim, uint32_t n_hidden_geo, uint32_t n_rgb_out, int dtype,
                                         uint64_t *bytes);
/* Field normals (additive; no counterpart kernel in the reference, whose grid network returns no normals: network_grid.py:177).
 * sigma = exp(raw + blob) with raw = MLP_den(MLP_net(enc))[0], so the surface normal is -grad_x(raw + blob) normalised; three kernels
 * give the chain's factors and the per-ray sums of renderer.py:428, :469-470.  The blob's gradient is the caller's.
 *
 * cnerf_field_density_grad: grad_enc [L, P, 2] FLOAT32 (8-byte aligned) = d raw / d enc for the first P samples of enc [L, stride, 2] (dtype,
 * kernel layout, enc_level_stride as in cnerf_field_forward_strided), and sigma [P] float32 (NULL: not wanted), bit-identical to the
 * forward's.  One backward pass through the two MLPs with upstream gradient 1, no weight gradients, no workspace, no atomics.
 * CNERF_F16 recomputes the forward with its roundings (the ReLU masks are the forward's) and rounds the gradient vector to half between
 * layers, fp32 accumulate; CNERF_F32 is exact float32.  Shapes as the forward: enc_dim even <= 64, n_hidden_geo 1 | 2, else CNERF_EINVAL. */
int cnerf_field_density_grad(const void *enc, const float *xyz, uint32_t P, uint32_t enc_dim, uint32_t n_hidden_geo, const float *params_net,
                             const float *params_den, float *sigma, float *grad_enc, int dtype, uint32_t enc_level_stride, void *stream);
/* grad_inputs [B, 3] float32 = sum_level sum_corner d w / d u * (embeddings[index] . grad_enc[level, b, :]), per unit-cube coordinate: what
 * gridencoder.cu:342-368 computes from a materialised dy_dx, without writing one.  inputs [B, 3] in [0, 1] (outside: zero, as the
 * forward's features); grad_enc [L, grad_level_stride, 2] float32, 8-byte aligned (0 = B).  fp32 accumulation, levels summed in order:
 * the same bits on every run.  The fused field's configuration only — D = 3, C = 2, interpolation 0 (linear), align_corners 0, gridtype
 * 0 | 1, L <= 32, embeddings of dtype CNERF_F32 | CNERF_F16 — anything else is CNERF_EINVAL. */
int cnerf_grid_encode_input_grad(const float *inputs, const void *embeddings, const int32_t *offsets_host, const float *grad_enc,
                                 float *grad_inputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, uint32_t gridtype,
                                 int align_corners, uint32_t interpolation, int dtype, uint32_t grad_level_stride, void *stream);
/* normal_map [V, N, 3] = sum_s w n and orient [V, N] = sum_s w max(0, n . d)^2 (the summand of loss_orient, renderer.py:428) with
 * n = -g / |g| (0 where |g|^2 < 1e-20: safe_normalize's epsilon) of g = grad_x [P, 3] read through src_index [N, S] (sorted position ->
 * row; NULL = identity, then N S <= P), weights [V, N, S] as cnerf_composite_run_indexed returns them (V = 1..3), dirs [N, 3].
 * Rows >= P count as zero normals.  Plain float32 in a fixed order. */
int cnerf_composite_normals(const float *weights, const int32_t *src_index, const float *grad_x, const float *dirs, uint32_t V, uint32_t N,
                            uint32_t S, uint32_t P, float *normal_map, float *orient, void *stream);

/* Packed weights (ABI 5).  Every launch above re-derives its fp16 MFMA fragment image of the three MLPs from the float32 parameters (14 us per
 * launch, three launches per training step).  cnerf_field_pack_weights writes that image once — `image`: 16-byte aligned device buffer of
 * cnerf_field_weight_image_bytes() bytes; the caller repacks after every change of the parameters — and the _img variants copy it into LDS
 * instead (CNERF_F16 only: with weight_image == NULL or CNERF_F32 they ARE cnerf_field_forward_strided / cnerf_field_backward_ex; the
 * narrow-encoding backward — enc_dim <= 16 — accepts an image and ignores it).  Results are bit-identical: the image holds the very halves
 * the kernels would have staged.  The reference has no counterpart (tcnn keeps fp16 parameters: network_grid.py:98-139). */
/* The table's optimiser step inside the backward scatter (ABI 5).  cnerf_grid_encode_backward* is where a table entry's gradient becomes final, and
 * cnerf_adam_step_scaled would read it back — with the parameter and both moments — a few launches later (62 us at the HBM roofline for the benchmark
 * table).  cnerf_grid_backward_adam(cfg) ARMS that step for the NEXT backward pass whose grad_embeddings == cfg->g (one shot; NULL disarms): if that
 * pass runs the histogram-free binned scatter (fp16, 3-D, C = 2) over ALL levels of the table (cfg->n floats), every entry leaves the pass updated
 * as cnerf_adam_step_scaled(p, g, m, v, p_half, n, lr, beta1, beta2, eps, scaler_state, extra_inv, zero_grad) would have left it — bit for bit, the
 * skip on found_inf included — and cnerf_grid_backward_adam_consumed() reports 1 (reads and clears); otherwise nothing is applied, it reports 0 and the
 * caller steps the table as usual.  The caller guarantees that this backward pass is the ONLY contribution to g in this optimiser step and that the
 * scaler's found_inf is final when the scatter runs (cnerf_scaler_watch covers the field's own producers).  Host-side switches, no launch.
 * No counterpart in the reference (torch.optim.Adam after loss.backward(): main.py:182, utils_init_nerf.py:608-616). */
typedef struct CnerfGridAdam {
    float *p, *g, *m, *v;            /* parameter, its gradient table, Adam moments: n floats each */
    void *p_half;                    /* fp16 shadow of p refreshed in the same pass, or NULL */
    uint64_t n;
    float lr, beta1, beta2, eps;
    const float *scaler_state;       /* float32[4] {scale, growth_tracker, found_inf, good_steps} (cnerf_scaler_*) */
    float extra_inv;                 /* extra factor on the un-scaling (1 / world_size) */
    int zero_grad;                   /* clear g after the update */
} CnerfGridAdam;
int cnerf_grid_backward_adam(const CnerfGridAdam *cfg);
int cnerf_grid_backward_adam_consumed(int *yes);

/* *id = the capture sequence id of `stream` while it is capturing into a hipGraph, 0 otherwise (host-side query, no launch): what a cache of
 * derived device data — e.g. the packed weights below — needs to know that a refresh it issues now is RECORDED, not executed. */
int cnerf_stream_capture_id(void *stream, uint64_t *id);
int cnerf_field_weight_image_bytes(uint32_t enc_dim, uint32_t n_hidden_geo, uint32_t n_rgb_out, uint64_t *bytes);
int cnerf_field_pack_weights(uint32_t enc_dim, uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                             const float *params_rgb, void *image, uint64_t image_bytes, void *stream);
int cnerf_field_forward_img(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                            uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                            const float *params_rgb, float *sigma, float *rgbc, int dtype, uint32_t enc_level_stride,
                            const void *weight_image, void *stream);
int cnerf_field_backward_img(const void *enc, const float *xyz, const float *dirs, uint32_t dir_group, uint32_t P, uint32_t enc_dim,
                             uint32_t n_hidden_geo, uint32_t n_rgb_out, const float *params_net, const float *params_den,
                             const float *params_rgb, const float *grad_sigma, const float *grad_rgbc, void *grad_enc,
                             float *grad_params_net, float *grad_params_den, float *grad_params_rgb, void *workspace,
                             uint64_t workspace_bytes, int dtype, const uint8_t *tile_live, const void *weight_image, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Generic fully fused MLP = tinycudann.Network(n_in, n_out, {FullyFusedMLP, ReLU, 64 neurons, 1|2 hidden layers})
 * (reference call sites: nerf/network_grid.py:18-54 RGB_network; :98-139 when the fused field is not used).
 * x [P, ldx] and y [P, ldy] row-major in `dtype` (leading dimensions in elements: strided views are accepted);
 * params float32 flat: row-major [64, pad16(n_in)], ([64,64]), [pad16(n_out), 64]; bias-free; output_activation 0 none | 1 sigmoid.
 * n_in <= 128, n_out <= 64, n_neurons == 64.  Numerics as cnerf_field_forward (CNERF_F16 = tcnn's, CNERF_F32 exact).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mlp_forward(const void *x, uint32_t ldx, const float *params, uint32_t P, uint32_t n_in, uint32_t n_out,
                      uint32_t n_neurons, uint32_t n_hidden_layers, int output_activation, void *y, uint32_t ldy, int dtype,
                      void *stream);
/* Backward (forward recomputed): grad_y [P, ldgy] (dtype) in; grad_x [P, ldgx] (dtype) out, NULL to skip;
 * grad_params float32, ACCUMULATED (caller pre-zeroes).  workspace: 16-byte aligned, cnerf_mlp_backward_workspace_bytes(). */
int cnerf_mlp_backward(const void *x, uint32_t ldx, const float *params, const void *grad_y, uint32_t ldgy, uint32_t P,
                       uint32_t n_in, uint32_t n_out, uint32_t n_neurons, uint32_t n_hidden_layers, int output_activation,
                       void *grad_x, uint32_t ldgx, float *grad_params, void *workspace, uint64_t workspace_bytes, int dtype,
                       void *stream);
int cnerf_mlp_backward_workspace_bytes(uint32_t P, uint32_t n_in, uint32_t n_out, uint32_t n_neurons,
                                       uint32_t n_hidden_layers, int dtype, uint64_t *bytes);

/* ------------------------------------------------------------------------------------------------
 * Ray generation (reference: nerf/provider.py:402-464 pinhole branch; nerf/provider_utils.py:239-302 get_rays)
 * c2w [V,3,4] row-major; outputs origins, directions [V, H, W, 3].
 * convention 0 = nerfstudio/OpenGL (provider.py: dir = normalize(R [ (x+.5-cx)/fx, -(y+.5-cy)/fy, -1 ]),
 *                 x = linspace(0, W*level-1, W), y likewise);
 * convention 1 = torch-ngp get_rays (dir = R normalize([ (i+.5-cx)/fx, (j+.5-cy)/fy, 1 ])), level ignored.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_generate_rays(const float *c2w, uint32_t V, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy,
                        float level, int convention, float *origins, float *directions, void *stream);
/* The OPENCV_FISHEYE branch of NerfstudioData._generate_rays (nerf/provider.py:421-433): the nerfstudio pixel grid of convention 0, each
 * normalised coordinate un-distorted by radial_and_tangential_undistort (nerf/provider_utils.py:197-234: ten Newton steps on the residual /
 * Jacobian of :128-194, eps 1e-3), theta = clip(|coord|, 0, pi), dir = normalize(R [x sin(theta)/theta, y sin(theta)/theta, -cos(theta)]).
 * distortion_host: [k1, k2, k3, k4, p1, p2] (host array, as the reference's `distortion_params`, provider.py:359). */
int cnerf_generate_rays_fisheye(const float *c2w, uint32_t V, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy,
                                float level, const float *distortion_host, float *origins, float *directions, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Pure-PyTorch renderer `NeRFRenderer.run` (nerf/renderer.py:278-405) as fused kernels.
 * ---------------------------------------------------------------------------------------------- */
/* sample_pdf — nerf/renderer.py:21-55 for arbitrary bins / weights (run() itself uses the fused cnerf_sample_fine_merge): bins [B, n_bins],
 * weights [B, n_bins - 1] -> samples [B, n_samples]; pdf = (w + 1e-5) / sum, cdf = [0, cumsum(pdf)], searchsorted(right=True), lerp with
 * denom < 1e-5 -> 1.  u [B, n_samples] replays the torch.rand draw of :37; NULL = det (the midpoint linspace of :33-35).  n_bins <= 256. */
int cnerf_sample_pdf(const float *bins, const float *weights, const float *u, uint32_t B, uint32_t n_bins, uint32_t n_samples,
                     float *samples, void *stream);
/* Stratified sampling: z = near + (far-near) * linspace(0,1,T)[i] + (noise-0.5)*sample_dist (noise NULL = no
 * perturbation), xyz = clip(o + d z, aabb)  (renderer.py:310-322).  z_vals [N,T], xyzs [N,T,3]. */
int cnerf_sample_coarse(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb,
                        const float *noise, uint32_t N, uint32_t T, float *z_vals, float *xyzs, void *stream);
/* Importance resampling + merge (renderer.py:334-363 + sample_pdf :21-55): from coarse z [N,T] and sigma [N,T]
 * computes weights, inverts the CDF at u [N,t] (u NULL = deterministic midpoints, sample_pdf:34), and writes the
 * merged, sorted z_all [N,T+t] and xyz_all [N,T+t,3].  T, t <= 128. */
int cnerf_sample_fine_merge(const float *rays_o, const float *rays_d, const float *nears, const float *fars,
                            const float *aabb, const float *z_vals, const float *sigmas, const float *u, uint32_t N,
                            uint32_t T, uint32_t t, float *z_all, float *xyz_all, void *stream);
/* Split form of the same step: the new samples are NOT merged into the coarse ones in memory.  z_all [N,T+t] is the sorted merge as
 * above; xyz_fine [N,t,3] receives the new samples in their own block; src_index [N,T+t] (uint32) maps every sorted position to its
 * row in the sample list [coarse block N*T rows | fine block N*t rows]: coarse i of ray n -> n*T + i, fine m (draw order) -> N*T + n*t + m.
 * The field is then evaluated on that list (the coarse block's grid features are already there from the density pass) and the
 * compositing entries below read through src_index.  xyz_all may be NULL here (or non-NULL to get both forms).
 * For every float input — a ray looking away from the box (far < near: descending z_vals), a NaN near, NaN or infinite sigmas — row n of
 * src_index is a permutation of ray n's rows, every output element is written and z_all is in sort order, ascending with NaN last: the
 * compositing backward stores through src_index and relies on it. */
int cnerf_sample_fine_merge_split(const float *rays_o, const float *rays_d, const float *nears, const float *fars,
                                  const float *aabb, const float *z_vals, const float *sigmas, const float *u, uint32_t N,
                                  uint32_t T, uint32_t t, float *z_all, float *xyz_all, float *xyz_fine, uint32_t *src_index,
                                  void *stream);
/* The same two samplers also writing the grid's [0,1] coordinates of their points, unit = (xyz + bound) / (2 bound) — the map
 * GridEncoder.forward applies first (gridencoder/grid.py:156) — so that the gather needs no elementwise pass in between.
 * unit [N,T,3] / unit_fine [N,t,3] float32, same arithmetic as the torch expression on a GPU (float add, then a multiplication by the
 * float reciprocal of 2*bound: that is how torch divides a tensor by a host scalar). */
int cnerf_sample_coarse_unit(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb,
                             const float *noise, uint32_t N, uint32_t T, float *z_vals, float *xyzs, float *unit, float bound,
                             void *stream);
/* cnerf_sample_coarse_unit with cnerf_near_far_from_aabb folded in (renderer.py:297 then :309-322: one launch instead of two): nears / fars
 * [N] are OUTPUTS here, computed per ray against `aabb` with the arithmetic of raymarching.cu:91-145 (bit-identical to the separate call). */
int cnerf_sample_coarse_unit_aabb(const float *rays_o, const float *rays_d, const float *aabb, float min_near, const float *noise, uint32_t N,
                                  uint32_t T, float *nears, float *fars, float *z_vals, float *xyzs, float *unit, float bound, void *stream);
int cnerf_sample_fine_merge_split_unit(const float *rays_o, const float *rays_d, const float *nears, const float *fars,
                                       const float *aabb, const float *z_vals, const float *sigmas, const float *u, uint32_t N,
                                       uint32_t T, uint32_t t, float *z_all, float *xyz_fine, uint32_t *src_index,
                                       float *unit_fine, float bound, void *stream);
/* weights_sum_i x3 (renderer.py:384-402, 407-474) in one pass over [N,S] samples: all / fg (sigma*edit_mask) /
 * bg (sigma*(1-edit_mask)) composites.  soft_mask: edit = sigmoid((conf-thr)*100) else conf>0.5.
 * rgbc [N,S,4] (rgb + confidence), sigmas [N,S], z_vals [N,S].
 * out_ray [3][N][6]  = per composite (all,fg,bg): image rgb, depth, weights_sum, render_mask;
 * out_weights [3][N][S] (NULL to skip). */
int cnerf_composite_run(const float *sigmas, const float *rgbc, const float *z_vals, const float *nears, const float *fars,
                        uint32_t N, uint32_t S, uint32_t num_steps, int soft_mask, float conf_thr, float *out_ray,
                        float *out_weights, void *stream);
/* Backward of cnerf_composite_run: grad_out_ray [3][N][6] -> grad_sigmas [N,S], grad_rgbc [N,S,4]
 * (depth and weights_sum gradients are honoured; detach_* flags follow renderer.py:409-418, 460-463). */
int cnerf_composite_run_backward(const float *grad_out_ray, const float *sigmas, const float *rgbc, const float *z_vals,
                                 const float *nears, const float *fars, uint32_t N, uint32_t S, uint32_t num_steps,
                                 int soft_mask, float conf_thr, int detach_bg, int detach_mask_from_field,
                                 float *grad_sigmas, float *grad_rgbc, void *stream);
/* Indexed forms: sample n,i (sorted position) lives at row src_index[n*S+i] of sigmas / rgbc / grad_* (NULL = row n*S+i, i.e. the
 * plain forms).  sigma_sorted [N,S] / rgbc_sorted [N,S,4] (may be NULL) receive the per-sample inputs in sorted order — the
 * `sigma` / `rgbs` entries of run()'s result dict (renderer.py:396-398). */
int cnerf_composite_run_indexed(const float *sigmas, const float *rgbc, const float *z_vals, const float *nears, const float *fars,
                                uint32_t N, uint32_t S, uint32_t num_steps, int soft_mask, float conf_thr,
                                const uint32_t *src_index, float *out_ray, float *out_weights, float *sigma_sorted,
                                float *rgbc_sorted, void *stream);
/* cnerf_composite_run_indexed computing only the variants whose bit is set in variant_mask (bit 0 all, 1 edit region, 2 background; 7 = all three):
 * the rows of out_ray (and of out_weights, when given) that belong to the others are written as zeros.  The reconstruction stage reads the first
 * composite only (utils_init_nerf.py:214-260 `train_step`); the editing stage all three. */
int cnerf_composite_run_indexed_variants(const float *sigmas, const float *rgbc, const float *z_vals, const float *nears, const float *fars,
                                         uint32_t N, uint32_t S, uint32_t num_steps, int soft_mask, float conf_thr, const uint32_t *src_index,
                                         float *out_ray, float *out_weights, float *sigma_sorted, float *rgbc_sorted, uint32_t variant_mask,
                                         void *stream);
int cnerf_composite_run_backward_indexed(const float *grad_out_ray, const float *sigmas, const float *rgbc, const float *z_vals,
                                         const float *nears, const float *fars, uint32_t N, uint32_t S, uint32_t num_steps,
                                         int soft_mask, float conf_thr, int detach_bg, int detach_mask_from_field,
                                         const uint32_t *src_index, float *grad_sigmas, float *grad_rgbc, void *stream);
/* The same with early termination for a half-precision consumer (round 5; the reference's own early-out is `T < T_thresh` in
 * raymarching.cu:691-772, its run() path has none).  flush_half_zero: a sample whose gradients AS THE FUSED FIELD BACKWARD CONSUMES THEM —
 * half(g_sigma * exp'(raw)), half(g_c * sigmoid'(c)) — are all zero (|g_sigma| sigma < 2^-26 and |g_c| c (1 - c) < 2^-26: behind an opaque
 * surface, in empty space) gets exact zeros in grad_sigmas / grad_rgbc: every parameter gradient computed downstream is bit-identical, and the
 * field backward / grid scatter can skip the row.  tile_live (optional, uint8 [N * S / 32]; needs src_index and num_steps, S - num_steps
 * multiples of 32): byte k = 1 when rows 32 k .. 32 k + 31 of the sample list hold at least one live row (cnerf_field_backward_ex). */
int cnerf_composite_run_backward_indexed_flush(const float *grad_out_ray, const float *sigmas, const float *rgbc, const float *z_vals,
                                               const float *nears, const float *fars, uint32_t N, uint32_t S, uint32_t num_steps,
                                               int soft_mask, float conf_thr, int detach_bg, int detach_mask_from_field,
                                               const uint32_t *src_index, float *grad_sigmas, float *grad_rgbc, int flush_half_zero,
                                               uint8_t *tile_live, void *stream);

/* Ray regularisers (additive, same ABI version): two losses on how a ray's weight is distributed along the ray, per composite variant, from the
 * same inputs and with the same w / alpha / T / delta as cnerf_composite_run_indexed (src_index NULL = rows in sorted order).  With
 * L = far - near, d_i = delta_i / L, m_i = (z_i - near) / L + d_i / 2:
 *   out_reg[v][n][0] = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i                          (distortion loss of mip-NeRF 360)
 *   out_reg[v][n][1] = -sum_i p_i log(p_i + 1e-10), p = w / (W + 1e-10), W = sum w, if W > min_opacity, else 0     (ray entropy of InfoNeRF)
 * out_reg is float [3][N][2]; rows of variants outside variant_mask (bit 0 all, 1 edit region, 2 background) are zeros.  O(S) per ray by prefix
 * sums: z_vals must be non-decreasing along each ray (cnerf_sample_fine_merge's output is).  A ray with !(far > near) gives exact zeros, never
 * a NaN.  1 <= S <= 256, num_steps >= 1 (the last interval is (far - near) / num_steps). */
int cnerf_ray_reg_forward(const float *sigmas, const float *rgbc, const float *z_vals, const float *nears, const float *fars, uint32_t N,
                          uint32_t S, uint32_t num_steps, int soft_mask, float conf_thr, const uint32_t *src_index, uint32_t variant_mask,
                          float min_opacity, float *out_reg, void *stream);
/* Its gradient: grad_reg float [3][N][2] -> grad_sigmas [P] and, when grad_rgbc is given (16-byte aligned; NULL where nothing depends on the
 * confidence: hard mask, or variant 0 only), grad_rgbc [P][4] with zeros in the rgb lanes.  Every row is written; z_vals / nears / fars are
 * constants and the min_opacity gate is one too.  detach_bg as in cnerf_composite_run_backward.  A variant outside variant_mask, or whose two
 * incoming gradients are both zero, is skipped.  No atomics: the result is bit-reproducible. */
int cnerf_ray_reg_backward(const float *grad_reg, const float *sigmas, const float *rgbc, const float *z_vals, const float *nears,
                           const float *fars, uint32_t N, uint32_t S, uint32_t num_steps, int soft_mask, float conf_thr, int detach_bg,
                           const uint32_t *src_index, uint32_t variant_mask, float min_opacity, float *grad_sigmas, float *grad_rgbc,
                           void *stream);

/* Loss of the reconstruction step (Trainer_Nerf.train_step_pretrain, utils_init_nerf.py:220-234) with its gradient, one launch:
 *   loss = w_rgb * mean((image - rgb_gt)^2) + w_conf * mean((render_mask - mask_gt)^2)
 * on the `all` composite of out_ray [3][N][6] (cnerf_composite_run); rgb_gt [N,3], mask_gt [N] (NULL: no mask term).
 * loss float32[65]: loss[0] = the loss, loss[1..64] = scratch (per-workgroup partial sums, added in a fixed order);
 * grad_out_ray [3][N][6] = d(loss)/d(out_ray), ready for cnerf_composite_run_backward. */
int cnerf_recon_loss(const float *out_ray, const float *rgb_gt, const float *mask_gt, uint32_t N, float w_rgb, float w_conf,
                     float *loss, float *grad_out_ray, void *stream);
/* the same with grad_out_ray multiplied by the device scalar grad_scale[0] — the seed the backward pass starts from under a loss scaler
 * (GradScaler.scale(loss).backward()): the element-wise multiply of the autograd node disappears.  grad_scale NULL = plain. */
int cnerf_recon_loss_scaled(const float *out_ray, const float *rgb_gt, const float *mask_gt, uint32_t N, float w_rgb, float w_conf,
                            const float *grad_scale, float *loss, float *grad_out_ray, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step used by the reference's recipe (main.py:182: Adam betas (0.9,0.99) eps 1e-15, no weight decay),
 * fused with gradient un-scaling, the fp16 shadow-table refresh and gradient zeroing.
 * p, m, v float32 [n]; g float32 [n] (zeroed after use if zero_grad); p_half (may be NULL) float16 [n].
 * step = 1-based step index (bias correction on the host); g is multiplied by grad_scale_inv first.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_adam_step(float *p, float *g, float *m, float *v, void *p_half, uint64_t n, float lr, float beta1, float beta2,
                    float eps, uint32_t step, float grad_scale_inv, int zero_grad, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Dynamic loss scaling with torch.cuda.amp.GradScaler's semantics (the reference trainer's fp16 recipe:
 * `self.scaler = GradScaler(enabled=fp16)`, scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()),
 * kept on the device so that a training step has no host read:
 *   state = float32[4] {scale, growth_tracker, found_inf, good_steps}  (initialise to {65536, 0, 0, 0}).
 * cnerf_scaler_check     : found_inf |= any non-finite value in g[0..n)  (call on the all-reduced gradients).
 * cnerf_adam_step_scaled : cnerf_adam_step with g multiplied by extra_inv / scale, the 1-based step = good_steps + 1 (bias
 *                          correction in the kernel) and the whole update skipped when found_inf is set (gradients are still
 *                          zeroed if zero_grad) — what scaler.step() does.
 * cnerf_scaler_update    : found_inf ? {scale *= backoff, tracker = 0} : {good_steps += 1, tracker += 1, tracker == interval ?
 *                          {scale *= growth, tracker = 0}}; found_inf = 0.  Call once per step after every adam_step_scaled.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_scaler_check(const float *g, uint64_t n, float *state, void *stream);
/* Round 6: while a scaler state is WATCHED (state != NULL; NULL switches it off — the default), the two gradient-producing entry points of the
 * field raise its found_inf themselves on their launch stream: cnerf_field_backward* when a parameter gradient it writes is not finite (every
 * form, the two-launch fallback of wide encodings and of float32 included: all of them add their partial weight gradients in one reduction that checks),
 * cnerf_grid_encode_backward* when an incoming feature gradient is not finite (the value it then also poisons the table gradient with).  A caller
 * whose gradients ALL come from these entry points may skip cnerf_scaler_check (a pass over every gradient: 9 us for the benchmark table, 30 us
 * for the reference field's).  One watched state per process; host-side switch, no launch. */
int cnerf_scaler_watch(float *state);
int cnerf_adam_step_scaled(float *p, float *g, float *m, float *v, void *p_half, uint64_t n, float lr, float beta1, float beta2,
                           float eps, const float *state, float extra_inv, int zero_grad, void *stream);
int cnerf_scaler_update(float *state, float growth_factor, float backoff_factor, uint32_t growth_interval, void *stream);
/* cnerf_adam_step_scaled for up to CNERF_ADAM_MAX_JOBS SMALL tensors in one single-workgroup launch (the reference's three tinycudann
 * parameter vectors: main.py:182 gives each network its own Adam group) and, with update_scaler != 0, cnerf_scaler_update folded into
 * its tail — call it as the LAST adam step of the iteration.  Plain pointers, no alignment demands. */
#define CNERF_ADAM_MAX_JOBS 8
typedef struct CnerfAdamJobs {
    float *p[CNERF_ADAM_MAX_JOBS], *g[CNERF_ADAM_MAX_JOBS], *m[CNERF_ADAM_MAX_JOBS], *v[CNERF_ADAM_MAX_JOBS];
    void *p_half[CNERF_ADAM_MAX_JOBS];            /* optional fp16 shadows (NULL) */
    uint64_t n[CNERF_ADAM_MAX_JOBS];
    float lr[CNERF_ADAM_MAX_JOBS];
    uint32_t n_jobs;
} CnerfAdamJobs;
int cnerf_adam_step_scaled_multi(const CnerfAdamJobs *jobs, float beta1, float beta2, float eps, float *state, float extra_inv, int zero_grad,
                                 int update_scaler, float growth_factor, float backoff_factor, uint32_t growth_interval, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange (customnerf_amd/dp.py; the reference has no working multi-GPU path: its DDP scaffolding
 * is dead code, nerf/utils_init_nerf.py:76-78, 709-726 — SURVEY.md §8e).  The collectives themselves are RCCL's; these are
 * the two passes either side of the all-to-all.
 * cnerf_dp_pack   : payload[i] = half(grad[i] * scale), grad[i] = 0   (grad 16-byte aligned, payload 8-byte aligned)
 * cnerf_dp_reduce : out[i] = sum_r float(recv[r * shard + i]), r < world, accumulated in float32; shard % 64 == 0;
 *                   scaler_state (nullable): found_inf |= any non-finite sum — cnerf_scaler_check folded in.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_dp_pack(float *grad, void *payload_half, uint64_t n, float scale, void *stream);
int cnerf_dp_reduce(const void *recv_half, uint32_t world, uint64_t shard, float *out, float *scaler_state, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Marching cubes over a dense volume (mesh export: customnerf_amd/mesh.py; the reference's convert_sigma_samples_to_ply,
 * nerf/renderer.py:128-196, calls skimage.measure.marching_cubes on the host).
 * vol float32 [nx][ny][nz] (z fastest, meshgrid('ij') order); corner inside <=> v >= level (NaN: outside); one vertex per crossing edge
 * (p, p + e_axis), owned by p.  Case table: csrc/mc_tables.h (generated by csrc/gen_mc_tables.py; crack-free for any input).
 *   workspace_bytes : bytes of the workspace `ws` (about 6 per grid point).  nx, ny, nz >= 2 and nx * ny * nz < 2^31, else CNERF_EINVAL.
 *   count           : counts[2] (device uint32) = (vertices, triangles); both 0xffffffff if either exceeds INT32_MAX (emit then writes nothing).
 *                     ws (16-byte aligned, >= workspace_bytes, else CNERF_EINVAL) keeps the per-point state that emit reads.
 *   emit            : after count on the same stream with the same ws and level.  verts [V,3], normals [V,3] (NULL: none), faces [F,3] int32;
 *                     entries at or past max_verts / max_faces are not written (verts / faces may be NULL when their max is 0).
 *                     Vertices in (linear point index, axis) order: t = clamp((level - v0) / (v1 - v0), 0, 1) (NaN t: 0.5),
 *                     pos = origin + (idx + t) * spacing on the crossing axis and origin + idx * spacing on the others.  Normals: -(g0 + t (g1 - g0))
 *                     normalised, g = central differences of vol / spacing (one-sided on the volume's faces), i.e. towards lower values.
 *                     Triangles in (linear cell index, table order), winding (v1 - v0) x (v2 - v0) from inside to outside.
 * origin_host / spacing_host: float[3] on the host.  No atomics: the output is bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_marching_cubes_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz, uint64_t *bytes_host);
int cnerf_marching_cubes_count(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void *ws, uint64_t ws_bytes,
                               uint32_t *counts, void *stream);
int cnerf_marching_cubes_emit(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const float *origin_host,
                              const float *spacing_host, void *ws, uint64_t ws_bytes, float *verts, float *normals, int32_t *faces,
                              uint32_t max_verts, uint32_t max_faces, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Marching cubes over a brick-sparse volume (customnerf_amd/mesh.py sparse_volume / marching_cubes_sparse; csrc/mesh_sparse.hip; the
 * reference has none): the passes above over a list of n_bricks bricks of 8 x 8 x 8 lattice points in place of every point of an
 * nx x ny x nz lattice, so that a fine lattice costs memory and field evaluations only near the surface.  Same table, same arithmetic
 * (csrc/mesh_mc.h holds the one definition of both): where the bricks cover the surface the mesh is the dense one, bit for bit, in
 * another order.
 *   values float32 [n][512]: lattice point (x, y, z) lives in brick (x >> 3, y >> 3, z >> 3) at ((x & 7) 8 + (y & 7)) 8 + (z & 7);
 *                            entries past the lattice's end are never read.
 *   coords int32 [n][3]    : the bricks, unique and sorted lexicographically.
 *   nbr    int32 [n][27]   : index of the brick at offset (dx, dy, dz) in {-1, 0, 1}^3, slot (dx + 1) 9 + (dy + 1) 3 + dz + 1, or -1 when
 *                            it is not in the list (an index outside [0, n) counts as -1); slot 13 is the brick itself.
 * A point past the lattice's end does not exist (the dense pass's faces); a point inside it whose brick is absent is unavailable.
 *   workspace_bytes : bytes of `ws` (about 6 per point of the n bricks).  n_bricks < 2^22, else CNERF_EINVAL.
 *   count           : counts[3] (device uint32) = (vertices, triangles, open bricks); state (NULL: none) uint8 [n]: bit 0 the brick
 *                     crosses — an edge it owns with both ends available changes side, or a cell it owns with 8 available corners is
 *                     mixed; bit 1 it is complete — every one of its 26 neighbours that lies inside the lattice is in the list.  Only
 *                     complete bricks are meshed, the others add nothing to the counts; a crossing brick that is not complete is open.
 *                     Both counts 0xffffffff if either exceeds INT32_MAX.
 *   emit            : after count on the same stream with the same ws and arguments; writes nothing after an overflow or when any
 *                     brick is open.  verts / normals / faces as the dense emit; vertices in (brick index, local point index, axis)
 *                     order, triangles in (brick index, local cell index, table order); positions and gradients use the GLOBAL
 *                     lattice index, one-sided gradients at the lattice's faces only.  vert_keys (NULL: none) int64 [V] =
 *                     ((x ny + y) nz + z) 3 + axis of every vertex: sorting by it gives the dense pass's order.
 * n_bricks == 0: CNERF_OK without a launch.  Then NULL values / coords / nbr / ws / counts (emit: origin_host, spacing_host, verts or
 * faces with a non-zero max): CNERF_ENULL.  Then a dimension < 2 or > 2^20, n_bricks >= 2^22, ws short or not 16-byte aligned:
 * CNERF_EINVAL.  No atomics: the output is bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_marching_cubes_sparse_workspace_bytes(uint32_t n_bricks, uint64_t *bytes_host);
int cnerf_marching_cubes_sparse_count(const float *values, const int32_t *coords, const int32_t *nbr, uint32_t n_bricks, uint32_t nx,
                                      uint32_t ny, uint32_t nz, float level, void *ws, uint64_t ws_bytes, uint8_t *state, uint32_t *counts,
                                      void *stream);
int cnerf_marching_cubes_sparse_emit(const float *values, const int32_t *coords, const int32_t *nbr, uint32_t n_bricks, uint32_t nx,
                                     uint32_t ny, uint32_t nz, float level, const float *origin_host, const float *spacing_host, void *ws,
                                     uint64_t ws_bytes, float *verts, float *normals, int32_t *faces, int64_t *vert_keys, uint32_t max_verts,
                                     uint32_t max_faces, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh cleanup (customnerf_amd/mesh.py remove_small_components / simplify; csrc/mesh_clean.hip; the reference has none — NeRF-to-mesh tools
 * do it on the host).  Any triangle mesh: verts float32 [V][3], optional normals float32 [V][3] (NULL: none), faces int32 [F][3].
 * V, F < 2^31, else CNERF_EINVAL.  Two passes on `stream` like marching cubes: count writes counts[3] (device uint32) =
 * (vertices, faces, flags) — the one host read — and emit, after count on the same stream with the same ws and arguments, writes the
 * output; entries at or past max_verts / max_faces are not written (outputs may be NULL when their max is 0).  flags bit 0: some face
 * index lies outside [0, V); emit then writes nothing.  ws: 16-byte aligned, >= workspace_bytes, else CNERF_EINVAL.
 * The output does not depend on scheduling: integer atomics only, compaction by scan, input order kept.
 *
 * components : two vertices are connected when a face holds both; the label of a component is its smallest vertex index.  Component c is
 *              kept iff faces(c) >= min_faces and, when `largest` != 0, c has the most faces (the smaller label on a tie) and at least one.
 *              faces(c) counts the faces whose first vertex is in c; an unreferenced vertex is a 0-face component.  min_faces = 0 with
 *              largest = 0 keeps everything.  Kept vertices and faces keep their input order; faces are remapped to the new indices.
 *   workspace_bytes : about 12 bytes per vertex + 8 per 256 of max(V, F).
 *   emit            : verts_out [V'][3], normals_out [V'][3] (written when normals != NULL), faces_out [F'][3],
 *                     old_index [V'] int32 (NULL: none) = the input index of each output vertex.
 *
 * cluster    : vertex clustering with a quadric representative (Lindstrom 2000).  Grid grid_host[3] = (gx, gy, gz) >= 1 cells of edge
 *              cell_host[3] (finite, > 0) from origin_host[3] (finite), gx * gy * gz < 2^31, else CNERF_EINVAL.  The cluster of vertex p is
 *              clamp(floor((p - origin) / cell), 0, g - 1) per axis in float32 (NaN -> 0); output vertex i is the i-th occupied cell in
 *              linear order (x slowest, z fastest).  Its position: in the cell's frame u = (p - corner) / cell, x = xbar + A+ (-b - A xbar),
 *              xbar the members' mean, (A, b) the sum of a n n^T, a n d over the faces of nonzero area a with a vertex in the cluster (plane
 *              n . u + d = 0 through the face's first vertex), A+ without eigenvalues < 1e-3 of the largest; x clamped to [0, 1]^3.  Sums are
 *              64-bit fixed point (bounds: mesh_clean.hip).  Normals: the normalised sum of the members' normals.  Faces map to the clusters
 *              of their vertices in input winding; a face with two equal clusters is dropped, and of the faces with one unordered cluster
 *              triple only the first survives.  Survivors keep input order.
 *   workspace_bytes : 4 bytes per vertex + 5 per cell + 12 to 20 per face + 132 per possible cluster (min(V, G)).
 *   emit            : verts_out [K][3], normals_out [K][3] (written when normals != NULL), faces_out [F'][3].
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_components_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_components_count(const int32_t *faces, uint32_t V, uint32_t F, uint32_t min_faces, int largest, void *ws, uint64_t ws_bytes,
                                uint32_t *counts, void *stream);
int cnerf_mesh_components_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t min_faces,
                               int largest, void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out, int32_t *faces_out,
                               int32_t *old_index, uint32_t max_verts, uint32_t max_faces, void *stream);
int cnerf_mesh_cluster_workspace_bytes(uint32_t V, uint32_t F, const uint32_t *grid_host, uint64_t *bytes_host);
int cnerf_mesh_cluster_count(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, const float *origin_host, const float *cell_host,
                             const uint32_t *grid_host, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream);
int cnerf_mesh_cluster_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, const float *origin_host,
                            const float *cell_host, const uint32_t *grid_host, void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out,
                            int32_t *faces_out, uint32_t max_verts, uint32_t max_faces, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Quadric edge-collapse decimation to a target face count (customnerf_amd/mesh.py decimate; csrc/mesh_decimate.hip; Garland & Heckbert
 * 1997).  Input: verts float32 [V][3], faces int32 [F][3], edge-manifold and consistently oriented (an undirected edge in at most two faces,
 * which use it in opposite directions), no face repeating an index; zero-area faces are allowed.  V, F < 2^31 and F <= 0x55555555 (edge
 * ids 3 f + k fit 32 bits), else CNERF_EINVAL; ws 16-byte aligned and >= workspace_bytes(V, F of init), else CNERF_EINVAL.  The caller's
 * stream and workspace; no allocation, no host sync.  counts[4] (device uint32) = (referenced vertices, live faces, collapses in this call,
 * flags) is the one host read after init and after each round; F passed to _round / _emit is the live count of the last read (launch
 * grids shrink with the mesh).  flags bit 0: an index outside [0, V); bit 1: a non-manifold or inconsistently oriented edge; bit 2: a face
 * repeating an index.  After a flag, rounds and emit write nothing.
 *   init  : positions copied into ws; per vertex the quadric sum, in increasing face index, over its faces of nonzero area of
 *           area (n n^T, n d, d^2) in fp64, n the unit normal and d = -n . p0 from the float32 positions.
 *   round : one round of independent collapses.  A boundary vertex (on an edge with one face) never moves and is never removed.  Candidates:
 *           edges with two faces and at most one boundary endpoint; with one, the edge collapses onto it and is costed there; otherwise
 *           min(u, v) is kept at x = m + A+ (-b - A m) (m the midpoint, A+ by Jacobi without eigenvalues < 1e-3 lambda_max, x = m when A = 0).
 *           cost = x^T A x + 2 b^T x + c of Q_u + Q_v in fp64, clamped at 0, as float32; key = cost bits << 32 | (3 f + k), the canonical
 *           half-edge (f[k], f[k+1]) with f[k] < f[k+1].  Valid: both endpoints in <= 32 faces, exactly 2 shared neighbours, no two surviving
 *           faces around the kept vertex with one vertex set, no surviving face with n_old != 0 and n_new . n_old <= 0.2 |n_new||n_old|
 *           (n = (p1 - p0) x (p2 - p0), kept vertex at (float) x).  A valid edge whose key is the minimum at both endpoints and then at every
 *           vertex of every face around them wins; winners apply together, or, when they would take F below target_faces, only the
 *           ceil((F - target) / 2) smallest keys, so F' is target or target - 1.  The kept vertex gets (float) x and Q_u + Q_v, the two faces
 *           of the edge go, the others are remapped and compacted in order.  collapses = 0: no valid edge is left (or F <= target).
 *   emit  : verts_out [V'][3] the referenced vertices in increasing input index, old_index [V'] (NULL: none) their input indices,
 *           normals_out [V'][3] = normals[old_index] (written when normals != NULL), faces_out [F'][3] the surviving input faces in input
 *           order, remapped, winding kept.  Entries at or past max_verts / max_faces are not written (outputs may be NULL when their max is 0).
 *   workspace_bytes : about 127 bytes per vertex + 73 per face.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_decimate_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_decimate_init(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes,
                             uint32_t *counts, void *stream);
int cnerf_mesh_decimate_round(uint32_t V, uint32_t F, uint32_t target_faces, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream);
int cnerf_mesh_decimate_emit(const float *normals, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, float *verts_out,
                             float *normals_out, int32_t *faces_out, int32_t *old_index, uint32_t max_verts, uint32_t max_faces,
                             void *stream);

/* ------------------------------------------------------------------------------------------------
 * Texture atlas and baking (customnerf_amd/mesh.py atlas_layout / bake_texture; csrc/mesh_texture.hip; the reference writes positions only,
 * NeRF-to-mesh tools bake with xatlas + nvdiffrast on the host).  A trivial per-face-pair layout with no search, so every texel's owner
 * follows from its index; every face gets the same texels whatever its area (the area-proportional layout is the block after this one, the
 * chart-based layout the block after that; least-squares or angle-based unwrapping is not done).
 *   Image: R x R texels, 16 <= R <= 16384, RGB8 [R][R][3], row Y = image row (top first).  Pair p holds faces 2p (A) and 2p + 1 (B),
 *   P = ceil(F / 2); n = max(1, ceil(sqrt(P))) cells per row, s = floor(R / n) texels per cell edge, s >= 4 (else CNERF_EINVAL: decimate or
 *   raise R); F = 0 gives n = 1, s = R and no cell.  Pair p owns cell (cx, cy) = (p mod n, p div n); its local texel (i, j) is global
 *   texel (X, Y) = (cx s + i, cy s + j).  Cell texel index t = p s^2 + j s + i, t < P s^2.
 *   Corners (local texel centres): A (0, 0), (0, s-2), (s-2, 0); B (s-1, s-1), (s-1, 2), (2, s-1) — counter-clockwise with v up, like the
 *   faces.  Owner of local (i, j): A if i + j <= s - 1, else B; B of an odd F's last cell and the texels outside the first P cells are
 *   un-owned and get the fill colour.  Seam invariant: every texel with a nonzero bilinear weight at a point of a face's UV triangle is
 *   owned by that face (A reads i + j <= s-1 with i, j <= s-2; B reads i + j >= s with i, j >= 2), so nothing bleeds across faces or
 *   cells under bilinear filtering (mipmaps are not covered).
 *   UV of corner texel (X, Y), float32: u = (X + 0.5) / R, v = 1 - (Y + 0.5) / R.
 *   Texel -> surface point, unclamped (affine) barycentrics: A w1 = j / (s-2), w2 = i / (s-2); B w1 = (s-1-j) / (s-3), w2 = (s-1-i) / (s-3);
 *   p = p0 + w1 (p1 - p0) + w2 (p2 - p0) in float32, in this order, except at a corner texel, where p is that vertex (bit for bit).
 *   Texels beside the triangle extrapolate in its plane, so a colour affine in position is reproduced by bilinear lookup exactly, up to
 *   the uint8 rounding.  View direction d = -normalize(n0 + w1 (n1 - n0) + w2 (n2 - n0)) (the vertex normal at a corner texel); when
 *   that has zero (or non-finite) squared length, or normals is NULL, -normalize((p1 - p0) x (p2 - p0)); when that is zero too, (0, 0, -1).
 *   An un-owned cell texel gets x = (0, 0, 0), d = (0, 0, -1).
 * faces int32 [F][3], verts / normals float32 [V][3], V < 2^31.  The caller's stream; no allocation, no host sync, no float atomics.
 *   layout : host only: n_host, s_host, or CNERF_EINVAL.
 *   uvs    : uvs [F][3][2] (corner k of face f at [f][k]); entries of faces >= max_faces are not written.  Zeroes flags[0] (device uint32)
 *            first, then sets bit 0 when a face index lies outside [0, V): the one host read before baking; after it points and store
 *            write nothing.
 *   points : cell texels t in [t0, t1) (t1 <= P s^2, else CNERF_EINVAL): x [N][3] and d [N][3] at row t - t0; rows >= max_points are not
 *            written.  normals may be NULL.
 *   store  : rgb float32 rows [N] of rgb_stride >= 3 floats (first three used) for t in [t0, t1) -> round(clamp(rgb, 0, 1) * 255) (half to
 *            even, NaN -> 0) at the texel's global position; an un-owned cell texel gets fill_host[3] (uint8 on the host).
 *   fill   : fill_host on every texel outside the first P cells (what store does not write).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_atlas_layout(uint32_t F, uint32_t R, uint32_t *n_host, uint32_t *s_host);
int cnerf_mesh_atlas_uvs(const int32_t *faces, uint32_t V, uint32_t F, uint32_t R, float *uvs, uint32_t max_faces, uint32_t *flags,
                         void *stream);
int cnerf_mesh_atlas_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, uint32_t t0,
                            uint32_t t1, const uint32_t *flags, float *x, float *d, uint32_t max_points, void *stream);
int cnerf_mesh_atlas_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                            const float *tangents, uint32_t t0, uint32_t t1, const float *m, uint32_t m_stride, const uint32_t *flags, float *rgb,
                            uint32_t max_points, void *stream);
int cnerf_mesh_atlas_store(uint32_t F, uint32_t R, uint32_t t0, uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host,
                           const uint32_t *flags, uint8_t *image, void *stream);
int cnerf_mesh_atlas_fill(uint32_t F, uint32_t R, const uint8_t *fill_host, uint8_t *image, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Area-proportional texture atlas (customnerf_amd/mesh.py atlas_plan / bake_texture(layout='area'); csrc/mesh_texture.hip; restatement:
 * tests/atlas_sized_restatement.py).  A face gets a square cell of 4 * 2^k texels, k from its longest edge; cells lie along a Z-order curve,
 * largest first.  Still search-free: the owner of a texel follows from its index and a table of at most eight numbers, and inside a cell
 * every rule of the block above holds with the cell's own s, the seam invariant included.
 *   Size key of a face, float32 without sqrt (the build has -ffp-contract=off): for the edges (0,1), (1,2), (2,0), l = (dx dx + dy dy) + dz dz
 *   of the float32 differences p_b - p_a; L2 = the maximum of the three (a NaN beside a number is ignored); key = float_bits(L2) >> 20 when
 *   L2 is finite and > 0, else 0.  0 <= key <= 2047: 16 keys per octave of edge length.
 *   Classes: R a power of two in [16, 16384] (else CNERF_EINVAL); K = min(7, log2(R) - 2); class k has cells of edge s_k = 4 * 2^k texels,
 *   4^k tiles of 4 x 4 texels.  For a threshold e in [0, 2048]: k_f = 0 if key_f < e, else min((key_f - e) >> 4, K).  n_k faces in class k,
 *   C_k = ceil(n_k / 2) cells, tiles(e) = sum_k C_k 4^k.  e = the smallest value with tiles(e) <= (R / 4)^2, found by going up from 0
 *   (tiles(e) falls as e rises except that a face moving down a class can open one more cell there; it is not monotone); when even
 *   tiles(2048) = ceil(F / 2) does not fit: CNERF_EINVAL (decimate or raise R).  F = 0 gives e = 0 and no cell.  F <= 2^25.
 *   Cells: the rank r_f of face f = the number of faces g < f with k_g = k_f (face order); cell c = r_f >> 1 of its class, b = r_f & 1
 *   (0: A, 1: B).  Classes are laid out from K down to 0: class tile offset O_k = sum_{k' > k} C_k' 4^k', the cell's tile offset
 *   o = O_k + c 4^k, its tile (tx, ty) = (even bits of o, odd bits of o), its origin texel (X0, Y0) = (4 tx, 4 ty).  Sizes descend along
 *   the curve, so every cell is aligned to its own size; cells are disjoint and inside the image.  Cell texel index (the order texels are
 *   handed to the field in): t = T_k + c s_k^2 + j s_k + i with T_k = 16 O_k; t < 16 tiles(e) <= R^2.
 *   Inside a cell, with s = s_k: corners of A and B, owner of (i, j), u = (X0 + i + 0.5) / R, v = 1 - (Y0 + j + 0.5) / R, texel -> point
 *   and view direction with the corner-texel exception, all as above.  B of the last cell of a class with odd n_k is un-owned: x = 0,
 *   d = (0, 0, -1), the fill colour.  Texel (X, Y) lies in a cell iff interleave(X >> 2, Y >> 2) < tiles(e) (X's bits at the even
 *   positions); every other texel gets the fill colour.
 * The caller's stream and workspace (ws_bytes >= workspace_bytes(F), 16-byte aligned; it carries the keys from measure to plan and the
 * cell -> faces table from plan to points and store); no allocation, one host read (hist), integer atomics only, bit-reproducible.
 *   measure : hist (device uint32 [2049]) = the histogram of the keys in [0, 2048) and the flags in [2048]: bit 0 when a face index lies
 *             outside [0, V) (such a face is not counted).  The one host read; with a flag set plan, uvs, points and store write nothing.
 *   layout  : host only: hist_host[2048] -> e_host, counts_host[8] (n_k; 0 above K), tiles_host = tiles(e); or CNERF_EINVAL.
 *   plan    : for e and counts_host of layout: cells int32 [F][4] = (X0, Y0, s, b) per face (rows >= max_faces are not written) and the
 *             workspace's cell -> (face A, face B or -1) table.  flags = hist + 2048.  counts_host that are no partition of F, use a class
 *             above K or need more than (R / 4)^2 tiles are CNERF_EINVAL; a face whose rank is not below its class's count gets no cell.
 *   uvs     : uvs [F][3][2] from cells; faces >= max_faces are neither read nor written.
 *   points, store : as cnerf_mesh_atlas_points / _store for cell texels t in [t0, t1), t1 <= 16 tiles (else CNERF_EINVAL); a range may
 *             cross class boundaries.
 *   fill    : fill_host on every texel outside the cells (tiles = tiles_host of layout).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_atlas_sized_workspace_bytes(uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_atlas_sized_measure(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes,
                                   uint32_t *hist, void *stream);
int cnerf_mesh_atlas_sized_layout(const uint32_t *hist_host, uint32_t R, uint32_t *e_host, uint32_t *counts_host, uint32_t *tiles_host);
int cnerf_mesh_atlas_sized_plan(uint32_t F, uint32_t R, uint32_t e, const uint32_t *counts_host, void *ws, uint64_t ws_bytes,
                                const uint32_t *flags, int32_t *cells, uint32_t max_faces, void *stream);
int cnerf_mesh_atlas_sized_uvs(uint32_t F, uint32_t R, const int32_t *cells, const uint32_t *flags, float *uvs, uint32_t max_faces,
                               void *stream);
int cnerf_mesh_atlas_sized_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                                  const uint32_t *counts_host, void *ws, uint64_t ws_bytes, uint32_t t0, uint32_t t1,
                                  const uint32_t *flags, float *x, float *d, uint32_t max_points, void *stream);
int cnerf_mesh_atlas_sized_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R,
                                  const uint32_t *counts_host, void *ws, uint64_t ws_bytes, const float *tangents, uint32_t t0, uint32_t t1,
                                  const float *m, uint32_t m_stride, const uint32_t *flags, float *rgb, uint32_t max_points, void *stream);
int cnerf_mesh_atlas_sized_store(uint32_t F, uint32_t R, const uint32_t *counts_host, void *ws, uint64_t ws_bytes, uint32_t t0,
                                 uint32_t t1, const float *rgb, uint32_t rgb_stride, const uint8_t *fill_host, const uint32_t *flags,
                                 uint8_t *image, void *stream);
int cnerf_mesh_atlas_sized_fill(uint32_t R, uint32_t tiles, const uint8_t *fill_host, uint8_t *image, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Chart-based texture atlas (customnerf_amd/mesh.py chart_plan / bake_texture(layout='projected'); csrc/mesh_charts.hip; restatement:
 * tests/atlas_proj_restatement.py).  Faces are grouped into charts by the dominant axis of their normal, every chart is projected along
 * its axis (box projection: six large charts on a blob, stretch bounded by 2, no flipped face), the charts are shelf-packed at one texel
 * density, texels find their face by an exact rasterisation in UV space, and a gutter is grown round every chart.  Charts are not merged
 * across axes, the parameterisation is not relaxed, and charts that fold over themselves in projection are counted, not repaired.
 * verts / normals float32 [V][3], faces int32 [F][3], V <= 2^28, F <= 2^26, 16 <= R <= 16384 (any value), gutter g in [0, 8]; else CNERF_EINVAL.
 *   1. Class of a face, float32, one rounding per written operation: e1 = p1 - p0, e2 = p2 - p0, c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z,
 *      e1x e2y - e1y e2x) (as cnerf_mesh_smooth_normals), q = (cx cx + cy cy) + cz cz.  q not in (0, inf): class 6, no chart: UVs 0, no
 *      texel.  Axis of a vector: k = argmax |c_k|, ties to the lowest k (k = 0; k = 1 if |c1| > |c0|; k = 2 if |c2| > |c_k|); class
 *      2 k + (c_k < 0).  With normals: g = (n0 + n1) + n2 per component; when every component is finite and one is nonzero, (k', s') = the
 *      axis and sign of g; the face takes class 2 k' + s' iff (c_k' < 0) == s' and 4 (c_k' c_k') >= q (|n . axis| >= 0.5); otherwise, and
 *      without normals, it keeps its own class.  A face index outside [0, V) sets flag bit 0; after that no pass writes anything.
 *   2. Charts: faces of one class that share a vertex are one chart: union-find over the nodes 6 v + class, uniting the three nodes of every
 *      classed face; a component's root is its smallest node.  Chart index = rank of the root among the roots of the nodes that a face
 *      uses, in increasing order; C charts, C <= F.  face_chart = -1 for class 6.
 *   3. Projection: class (k, +): (a, b) = (x[(k+1)%3], x[(k+2)%3]); class (k, -): (a, b) = (x[(k+2)%3], x[(k+1)%3]): a classed face is
 *      counter-clockwise in (a, b) with b up.  Extents of a chart: a0 / a1 = min / max of a over the corners of its faces, b0 / b1 alike, by
 *      integer atomics on the order-preserving image of the float (bits with the sign bit set, or all bits inverted for a negative: -0 < +0).
 *   4. Density and packing (host, fp64, cnerf_mesh_atlas_proj_pack).  At density rho chart c needs w = ceil(rho (a1 - a0)) + 1 + 2 g by
 *      h = ceil(rho (b1 - b0)) + 1 + 2 g texels (the differences of the float32 extents in fp64).  fits(rho): every w, h <= R; the charts in
 *      the order h descending, then w descending, then index ascending; x = y = 0, the shelf's height H = the first chart's h; per chart: if
 *      x + w > R then y += H, x = 0, H = h; if y + H > R it does not fit; the chart's rectangle is (X0, Y0, w, h) = (x, y, w, h); x += w.
 *      rho = 0 must fit, else CNERF_EINVAL (more than floor(R / (1 + 2 g))^2 charts: decimate or raise R).  D = the largest a1 - a0 or
 *      b1 - b0 of any chart; D = 0 gives rho = 0.  rho_hi = (R - 1 - 2 g) / D; if fits(rho_hi), rho = rho_hi; else lo = 0, hi = rho_hi and
 *      24 times: m = 0.5 (lo + hi), lo = m if fits(m) else hi = m; rho = lo.  fits is not monotone in rho under shelf packing; the rule is
 *      still well defined and returns a fitting rho.  An extent with a1 < a0, b1 < b0 or a non-finite difference is CNERF_EINVAL.
 *   5. UVs, fp64 in the order written, rounded to float32 once: tx = ((X0 + g) + 0.5) + rho (a - a0), ty = ((Y0 + h - 1 - g) + 0.5) -
 *      rho (b - b0) (texel space, rows from the top; texel (X, Y) has its centre at (X + 0.5, Y + 0.5)); u = tx / R, v = 1 - ty / R.
 *   6. Ownership, exact in int64.  Corners snapped to 1 / 256 texel: xi = rint(256 tx), yi = rint(256 ty) of the fp64 values (half to even);
 *      the centre of texel (X, Y) is (256 X + 128, 256 Y + 128).  As in the rasteriser's block below with the sign turned, because rows count
 *      from the top while the faces are counter-clockwise with v up: A = (y1 - y0)(x2 - x0) - (x1 - x0)(y2 - y0), and for corner k,
 *      i = (k + 1) % 3, j = (k + 2) % 3: E_k(px, py) = (yj - yi)(px - xi) - (xj - xi)(py - yi); E_0 + E_1 + E_2 = A.
 *      Pass A: a face with A > 0 covers the texels whose centre has every E_k >= 0 (edges inclusive; shared edges snap identically: no
 *      holes); candidates per axis ceil((min - 128) / 256) .. floor((max - 128) / 256), clamped to the image.  The owner is the smallest
 *      covering face index.  Pass B, only on texels un-owned after A: a face with A > 0 claims the texels X in ceil((min - 256) / 256) ..
 *      floor(max / 256) (Y alike, clamped to the image: the closed squares [256 X, 256 X + 256] that meet its box) with
 *      E_k(centre) + 128 (|xj - xi| + |yj - yi|) >= 0 for every k; a charted face with A <= 0 claims every texel of that range.  The
 *      smallest claiming index wins.  overlap_texels = the number of (face, texel) pairs with A > 0, every E_k > 0 at the centre and another
 *      face the owner after A.  The result does not depend on how the work is spread over threads (a face whose
 *      range has more than 1024 texels is covered by a workgroup).
 *   7. Gutter: g Jacobi rounds.  An un-owned texel takes the owner of its first owned neighbour inside the image in the order W, E, N, S, NW,
 *      NE, SW, SE (N = row Y - 1), read from the previous round's map.  Owned texels of a chart stay inside its rectangle, so growth never
 *      meets another chart.  Seam invariant for g >= 1: every texel with a nonzero bilinear weight at a point of a charted face's UV triangle
 *      is owned by a face of the same chart.
 *   8. Texel list: the owned texels after the gutter, numbered in row-major order, t in [0, total).  Point of texel t with owner f:
 *      w_k = (float) ((double) E_k / (double) A) at the texel's centre, unclamped; p = (p0 + w1 (p1 - p0)) + w2 (p2 - p0) in float32 (no
 *      corner exception); for an owner with A <= 0, p = p0 and w1 = w2 = 0.  d as cnerf_mesh_atlas_points with these weights: the
 *      interpolated normal, then the face normal, then (0, 0, -1).  Store: round(clamp(rgb, 0, 1) 255) as cnerf_mesh_atlas_store.
 * The caller's stream and workspace (16-byte aligned, >= workspace_bytes(V, F, R); it carries classes, charts, snapped corners, the owner map
 * and the texel list from pass to pass); no allocation, three host reads (counts; the C extents; totals), integer atomics only,
 * bit-reproducible.
 *   charts : counts (device uint32 [2]) is zeroed first; [1] = the flags, bit 0: an index outside [0, V); without a flag [0] = C,
 *            face_class / face_chart int32 [F] (rows >= max_faces are not written) and extents float32 [C][4] = (a0, a1, b0, b1) (rows >=
 *            max_charts are not written).  The host reads counts, then the C extents.  normals may be NULL.
 *   pack   : host only, no GPU needed: extents_host [C][4], R, g -> rho_host, rects_host int32 [C][4] = (X0, Y0, w, h), disjoint and inside
 *            the image; or CNERF_EINVAL.  A failed host allocation returns hipErrorOutOfMemory (2), never CNERF_EINVAL.
 *   raster : after charts on the same stream with the same ws, V, F, R; flags = counts + 1; rho and rects (device int32 [C][4]) of pack.
 *            uvs [F][3][2] (rows >= max_faces are not written), owner_ab int32 [R][R] (the map after A and B; may be NULL), owner int32
 *            [R][R] (after the gutter; -1: none), totals (device uint64 [2], zeroed first): [0] = total, [1] = overlap_texels — the last
 *            host read.  A face whose chart is not below C is treated as class 6.
 *   points : texels t in [t0, t1), t1 <= R^2 (else CNERF_EINVAL; t >= total writes nothing): x, d at row t - t0; rows >= max_points are not
 *            written.
 *   store  : rgb rows for t in [t0, t1) -> the texel's position in image [R][R][3].
 *   fill   : fill_host on every un-owned texel.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_atlas_proj_workspace_bytes(uint32_t V, uint32_t F, uint32_t R, uint64_t *bytes_host);
int cnerf_mesh_atlas_proj_charts(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, uint32_t *counts, int32_t *face_class, int32_t *face_chart, uint32_t max_faces,
                                 float *extents, uint32_t max_charts, void *stream);
int cnerf_mesh_atlas_proj_pack(const float *extents_host, uint32_t C, uint32_t R, uint32_t gutter, double *rho_host, int32_t *rects_host);
int cnerf_mesh_atlas_proj_raster(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, uint32_t gutter, double rho,
                                 const int32_t *rects, uint32_t C, void *ws, uint64_t ws_bytes, const uint32_t *flags, float *uvs,
                                 uint32_t max_faces, int32_t *owner_ab, int32_t *owner, uint64_t *totals, void *stream);
int cnerf_mesh_atlas_proj_points(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, uint32_t t0, uint32_t t1, const uint32_t *flags, float *x, float *d, uint32_t max_points,
                                 void *stream);
int cnerf_mesh_atlas_proj_tspace(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t R, void *ws,
                                 uint64_t ws_bytes, const float *tangents, uint32_t t0, uint32_t t1, const float *m, uint32_t m_stride,
                                 const uint32_t *flags, float *rgb, uint32_t max_points, void *stream);
int cnerf_mesh_atlas_proj_store(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, uint32_t t0, uint32_t t1, const float *rgb,
                                uint32_t rgb_stride, const uint32_t *flags, uint8_t *image, void *stream);
int cnerf_mesh_atlas_proj_fill(uint32_t V, uint32_t F, uint32_t R, void *ws, uint64_t ws_bytes, const uint8_t *fill_host,
                               const uint32_t *flags, uint8_t *image, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Welded vertices, tangent frames and tangent-space normal maps (customnerf_amd/mesh.py weld_corners / corner_tangents / gltf_vertices /
 * bake_texture(normal_map='tangent'); csrc/mesh_tangent.hip, k_bake_tspace of csrc/mesh_bake.h; restatement: tests/tangent_restatement.py).
 * What a glTF primitive and its normalTexture need.  verts / normals float32 [V][3], faces int32 [F][3], uvs float32 [F][3][2] (v up, as the
 * atlas passes write them); V < 2^31, F <= 0x2AAAAAAA, else CNERF_EINVAL.  Corner c = 3 f + k.  The caller's stream and workspace (16-byte
 * aligned, >= workspace_bytes(V, F), about 16 bytes per vertex + 60 per face); no allocation, no float atomics, every sum in a stated order:
 * bit-reproducible.  Red runs along +u and green along +v with v up (the OpenGL and glTF convention once v is flipped for the file).
 *   weld     : the key of a corner is (vertex index, bits of u, bits of v); corners with equal keys are one output vertex.  Output vertices
 *              are numbered by ascending vertex index and, within a vertex, by ascending smallest corner of the group.  corner_vertex int32
 *              [F][3] (rows >= max_faces are not written), vertex_corner int32 [W] (the smallest corner of each group; entries >= max_verts
 *              are not written; W <= 3 F), counts (device uint32 [2]) = (W, flags): the one host read.  flags bit 0: a face index outside
 *              [0, V); W is then 0 and weld, frames and vertices write nothing else.
 *   frames   : after weld on the same stream with the same ws, V, F, faces and uvs.  Per face, from float32 e1 = p1 - p0, e2 = p2 - p0,
 *              du1 = u1 - u0, dv1 = v1 - v0, du2 = u2 - u0, dv2 = v2 - v0, then in float64 with one rounding per written operation (products
 *              of two float32 values are exact): det = du1 dv2 - du2 dv1, s = -1 if det < 0 else 1, Tf = s (e1 dv2 - e2 dv1),
 *              Bf = s (e2 du1 - e1 du2), c = e1 x e2 (as cnerf_mesh_smooth_normals), A2 = sqrt((c0 c0 + c1 c1) + c2 c2), |x| =
 *              sqrt((x0 x0 + x1 x1) + x2 x2).  A face contributes unless det is 0 or non-finite or one of A2, |Tf|, |Bf| is not in
 *              (0, inf): (A2 Tf) / |Tf| to S_T, (A2 Bf) / |Bf| to S_B and c to S_N of the group of each of its corners; the sums start at
 *              0 and run in ascending corner index.  Per group: n = the vertex's normal read as float64, or S_N when normals is NULL,
 *              divided by sqrt(q), q = (n0 n0 + n1 n1) + n2 n2, when q is in (0, inf); else n = 0.  t = S_T - n (n . S_T) (dot products
 *              summed (a0 b0 + a1 b1) + a2 b2); when |t|^2 is not in [DBL_MIN, inf): t = c - n n_a, c the unit axis a of the smallest
 *              |n_a|, the lowest on ties (n = 0 gives t = (1, 0, 0)).  tangent xyz = (float) (t / sqrt(|t|^2)), w = -1 if
 *              (n x t) . S_B < 0 else +1.  tangents float32 [F][3][4]: every corner of a group gets the group's frame; rows >=
 *              max_faces are not written.  The workspace keeps (float) n per group for vertices.
 *   vertices : after frames.  For output vertex i with corner c = vertex_corner[i] of vertex v: positions [W][3] = verts[v], normals_out
 *              [W][3] = normals[v] as given, or the group's n when normals is NULL, uvs_out [W][2] = (u, 1 - v) of corner c in float32,
 *              tangents_out [W][4] = tangents[c]; indices uint32 [F][3] = corner_vertex.  W must be weld's (W > 3 F: CNERF_EINVAL).
 *   tspace   : cnerf_mesh_atlas_tspace / _sized_tspace / _proj_tspace, with the arguments of the layout's points pass: for cell texels
 *              [t0, t1) the float32 code rgb [N][3] (rows >= max_points are neither read nor written) of the object-space normals
 *              m [N][m_stride >= 3] in the texel's frame, for the layout's store pass.  N = -d of the points pass, bit for bit, with its
 *              weights w1, w2 and corner; float32, one rounding per written operation: T' = T0 + w1 (T1 - T0) + w2 (T2 - T0) of the corners'
 *              tangent xyz (a corner texel: that corner's), t = T' - N (N . T'); when |t|^2 is not in [FLT_MIN, inf): t = c - N N_a as
 *              above; t = t / sqrt(|t|^2); w = that of the corner with the largest of (1 - w1) - w2, w1, w2 (the lowest on ties; a corner
 *              texel: that corner's; a face without area in the layout: corner 0's); B = w (N x t); rgb = 0.5 + 0.5 (m . t, m . B, m . N).
 *              m == NULL encodes N itself: (0.5, 0.5, 1) exactly.  An un-owned cell texel gets (0.5, 0.5, 1); the fill colour of a
 *              tangent-space map is (128, 128, 255).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_tangent_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_tangent_weld(const int32_t *faces, const float *uvs, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts,
                            int32_t *corner_vertex, uint32_t max_faces, int32_t *vertex_corner, uint32_t max_verts, void *stream);
int cnerf_mesh_tangent_frames(const float *verts, const int32_t *faces, const float *uvs, const float *normals, uint32_t V, uint32_t F,
                              void *ws, uint64_t ws_bytes, float *tangents, uint32_t max_faces, void *stream);
int cnerf_mesh_tangent_vertices(const float *verts, const int32_t *faces, const float *uvs, const float *normals, const float *tangents,
                                const int32_t *corner_vertex, const int32_t *vertex_corner, uint32_t V, uint32_t F, uint32_t W, void *ws,
                                uint64_t ws_bytes, float *positions, float *normals_out, float *uvs_out, float *tangents_out,
                                uint32_t *indices, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Taubin lambda|mu smoothing with uniform weights and area-weighted vertex normals (customnerf_amd/mesh.py smooth / vertex_normals;
 * csrc/mesh_smooth.hip; Taubin 1995).  Any triangle mesh: verts float32 [V][3], faces int32 [F][3] (need not be manifold; a face repeating an
 * index adds only its distinct edges), optional normals float32 [V][3] (NULL: none).  V < 2^31 and F <= 0x2AAAAAAA (6 F neighbour records
 * fit 32 bits), else CNERF_EINVAL; ws 16-byte aligned and >= workspace_bytes(V, F), else CNERF_EINVAL.  The caller's stream and workspace;
 * no allocation, no host sync, integer atomics only (every list is sorted before it is read): the output is bit-reproducible.
 *   init    : from the faces alone: each vertex's neighbours (the distinct vertices sharing an edge with it, in increasing index), its faces
 *             (each once, in increasing index) and its boundary mark (one of its edges lies in exactly one face).  flags[0] (device uint32)
 *             = bit 0 when an index lies outside [0, V): the one host read; after it steps and normals write nothing.
 *   steps   : after init on the same stream with the same ws, V and F.  `iterations` of a lambda step and, when mu != 0, a mu step (lambda and
 *             mu finite, else CNERF_EINVAL); Jacobi: each step reads the previous positions only.  Step with factor s: a vertex with n > 0
 *             neighbours that is not pinned (pin_boundary != 0 pins boundary vertices) gets x + s * (m - x), m = sum / (float) n, sum = the
 *             neighbours' positions added in float32 in list order from the first, three rounded operations; every other vertex keeps x
 *             bit for bit.  The last step writes verts_out [V][3] (iterations = 0: a copy of verts_in), which must not overlap verts_in.
 *   normals : after init, from `verts` (any positions over the same faces): c = (p1 - p0) x (p2 - p0) per face in float32,
 *             (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); a = (0, 0, 0) + c of each of the vertex's faces in increasing face
 *             index; q = ax ax + ay ay + az az; 0 < q < inf: normals_out = a / sqrt(q) (correctly rounded), otherwise normals_in of the
 *             vertex, or (0, 0, 0) when normals_in is NULL.
 *   workspace_bytes : about 48 bytes per vertex + 36 per face.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_smooth_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_smooth_init(const int32_t *faces, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *flags, void *stream);
int cnerf_mesh_smooth_steps(const float *verts_in, uint32_t V, uint32_t F, uint32_t iterations, float lambda, float mu, int pin_boundary,
                            void *ws, uint64_t ws_bytes, float *verts_out, void *stream);
int cnerf_mesh_smooth_normals(const float *verts, const float *normals_in, uint32_t V, const int32_t *faces, uint32_t F, void *ws,
                              uint64_t ws_bytes, float *normals_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Mesh rasteriser: visibility buffer and shaded previews (customnerf_amd/mesh.py rasterize / render_mesh; csrc/mesh_raster.hip; the reference
 * has no rasteriser).  One pinhole camera per call, the cameras of cnerf_generate_rays.  All float arithmetic is float32, one rounding per
 * written operation, in the order written (the build has -ffp-contract=off); divisions and square roots are correctly rounded; rintf and
 * int64 -> float round to nearest even.
 *   Camera: c2w_host float32 [3][4] row-major ON THE HOST (m[r][k], t = column 3); fx, fy, cx, cy as in cnerf_generate_rays; convention 0 =
 *   'nerfstudio' (the camera looks down -z, y up), 1 = 'ngp' (+z forward, y down).  Pixel (ix, iy) is sampled at its centre
 *   (ix + 0.5, iy + 0.5), where both conventions of cnerf_generate_rays put the ray at level = 1.  Per vertex p: d = p - t,
 *   c_k = (m[0][k] d0 + m[1][k] d1) + m[2][k] d2; convention 0: z = -c_2, Y = cy + (-1) (fy (c_1 / z)); convention 1: z = c_2,
 *   Y = cy + fy (c_1 / z); both: X = cx + fx (c_0 / z).  Snapped to 1/256 pixel: xi = (int) rintf(X 256), yi = (int) rintf(Y 256); the centre
 *   of pixel ix is the fixed-point value 256 ix + 128.  q = 1 / z.
 *   Dropped faces: a face is dropped whole, never clipped, when one of its vertices has a non-finite z or z < near, a non-finite X or Y, or
 *   |rintf(X 256)| or |rintf(Y 256)| >= 2^28 (below it every edge function stays inside int64).  counts[0] counts them.  A dropped face
 *   leaves a hole, never a wrong pixel; near-plane clipping is not done.
 *   Coverage, exact in int64: A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) in pixel coordinates (x right, y down).  A == 0 covers nothing.
 *   A < 0 is front-facing: a mesh wound outwards (marching cubes) appears counter-clockwise on the screen.  cull 0 none, 1 back (skips
 *   A > 0), 2 front (skips A < 0).  For A < 0 vertices 1 and 2 are swapped, so that A > 0.  For vertex k, i = (k + 1) % 3, j = (k + 2) % 3:
 *   E_k = (xj - xi)(py - yi) - (yj - yi)(px - xi).  A pixel centre (px, py) is covered when for every k E_k > 0, or E_k == 0 and the edge is
 *   top-left: dy < 0, or dy == 0 and dx > 0, (dx, dy) = (xj - xi, yj - yi).  Candidate pixels per axis:
 *   ceil((min - 128) / 256) ... floor((max - 128) / 256), clamped to the image.
 *   Depth and winner: b_k = (float) E_k / (float) A, iz = (b0 q0 + b1 q1) + b2 q2 with each b_k q_k rounded, depth = 1 / iz (camera-axis
 *   depth).  The winner of a pixel is the covering face with the smallest 64-bit key (bits(depth) << 32) | face: the nearest, the lower index
 *   on a tie (depth is positive for near > 0, so the bit order is the numeric order).  Perspective-correct barycentrics of the winner:
 *   beta_k = (b_k q_k) depth, reported in the INPUT face's vertex order (the swap is undone).
 *   visibility : verts float32 [V][3], faces int32 [F][3]; per pixel in [H][W] row order: face_out int32 (-1: none), depth_out float32
 *            (+inf: none), bary_out float32 [3] (0: none).  counts (device uint32 [2]): [0] dropped faces, [1] flags, bit 0 = a face index
 *            lies outside [0, V) — the outputs are then all-empty; the one host read.  ws 16-byte aligned, >= workspace_bytes(V, F, H, W).
 *            F = 0 or H W = 0 is accepted (F = 0: every pixel is empty).
 *   shade  : from face / depth / bary of visibility (a face entry outside [0, F), or one whose indices lie outside [0, V), shades as a
 *            miss): image RGB8 [H][W][3], mask uint8 [H][W] (255 hit, 0 miss); a miss gets bg_host[3] (uint8 on the host).  mode
 *            0 vertex colours: colors uint8 [V][3], x = ((beta0 c0 + beta1 c1) + beta2 c2) / 255;
 *            1 texture: uvs float32 [F][3][2] (corner k of face f, v up) and texture RGB8 [R][R][3] (row 0 at the top, 1 <= R <= 16384) as
 *              cnerf_mesh_atlas_* make them: (u, v) = (beta0 uv0 + beta1 uv1) + beta2 uv2 per component, px = u R - 0.5,
 *              py = (1 - v) R - 0.5, X = floor(px), Y = floor(py), wx = px - X, wy = py - Y, texels clamped to the edge,
 *              x = (((1-wx)(1-wy) T[Y][X] + wx (1-wy) T[Y][X+1]) + (1-wx) wy T[Y+1][X]) + wx wy T[Y+1][X+1]) / 255;
 *            2 normals: a = (beta0 n0 + beta1 n1) + beta2 n2 (normals float32 [V][3]), l2 = (ax ax + ay ay) + az az; 0 < l2 < inf:
 *              n = a / sqrt(l2), else the same of (p1 - p0) x (p2 - p0) (verts), else n = 0; x = 0.5 + 0.5 n;
 *            3 depth: x = (depth - d0) / (d1 - d0) on the three channels.
 *            To uint8: round(clamp(x, 0, 1) 255), half to even, NaN -> 0, as cnerf_mesh_atlas_store does.  Buffers of other modes may be NULL.
 *   CNERF_EINVAL: fx or fy zero or non-finite, cx / cy / near non-finite, V, F or H W >= 2^31, convention, cull or mode out of range, a short or
 *   misaligned ws, R outside [1, 16384] in mode 1.  CNERF_ENULL: a required pointer is NULL.  Both return before any launch.
 *   The caller's stream and workspace; no allocation, no host sync; the only atomics are 64-bit integer minima on the key buffer and integer
 *   counters, so the output is bit-reproducible.  workspace_bytes: 8 bytes per pixel + 16 per vertex + 20 per face.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_raster_workspace_bytes(uint32_t V, uint32_t F, uint32_t H, uint32_t W, uint64_t *bytes_host);
int cnerf_mesh_raster_visibility(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, const float *c2w_host, float fx, float fy,
                                 float cx, float cy, uint32_t H, uint32_t W, int convention, float near, int cull, void *ws, uint64_t ws_bytes,
                                 int32_t *face_out, float *depth_out, float *bary_out, uint32_t *counts, void *stream);
int cnerf_mesh_raster_shade(const int32_t *face, const float *depth, const float *bary, uint32_t H, uint32_t W, const int32_t *faces, uint32_t V,
                            uint32_t F, int mode, const uint8_t *colors, const float *uvs, const uint8_t *texture, uint32_t R,
                            const float *verts, const float *normals, float d0, float d1, const uint8_t *bg_host, uint8_t *image, uint8_t *mask,
                            void *stream);

/* ------------------------------------------------------------------------------------------------
 * TSDF fusion: depth maps of a set of views fused into a truncated signed distance volume on marching cubes' lattice, whose zero level is
 * the surface the views show (customnerf_amd/mesh.py TSDFVolume; csrc/mesh_tsdf.hip; the reference has none — NeRF exporters do it on the
 * host).  All float arithmetic is float32, one rounding per written operation, in the order written (the build has -ffp-contract=off);
 * divisions and square roots are correctly rounded: the rasteriser's rules above.
 *   State: float32 [n][2] on the device, n = nx ny nz points in cnerf_marching_cubes_*'s order (z fastest): (acc, weight) = (sum of w s,
 *   sum of w) over the views integrated so far; all zero at first (the caller clears it).  origin_host / spacing_host float32 [3] on the
 *   host as cnerf_marching_cubes_emit takes them: lattice point idx sits at p_b = org_b + (float) idx_b sp_b.
 *   Cameras: those of cnerf_mesh_raster_visibility, one c2w_host float32 [3][4] per view ([n_views][3][4] on the host), shared fx, fy, cx,
 *   cy, convention and near; the vertex transform is the rasteriser's own code (csrc/mesh_camera.h).
 *   integrate, per point, for each view v in index order:
 *      1. d = p - t                          2. c_k = (m[0][k] d0 + m[1][k] d1) + m[2][k] d2
 *      3. z = -c_2 (convention 0) or c_2 (convention 1)             4. skip unless z >= near (a NaN z fails the test)
 *      5. X = cx + fx (c_0 / z)              6. Y = cy + (-1) (fy (c_1 / z)) (convention 0) or cy + fy (c_1 / z) (convention 1)
 *      7. skip unless 0 <= X < (float) W and 0 <= Y < (float) H, tested on the floats (non-finite values fail)
 *      8. ix = (int) floorf(X), iy = (int) floorf(Y): the pixel whose centre (ix + .5, iy + .5) carries that ray; skip unless ix < W and
 *         iy < H (which can fail only where (float) W rounds up, W > 2^24)
 *      9. D = depth[v][iy][ix]; skip if D is NaN or D <= 0.  +inf is valid: nothing was hit, the ray is free space all the way
 *     10. w = pixel_weight ? pixel_weight[v][iy][ix] : 1; skip unless 0 < w < inf
 *     11. r = z (depth_kind 0: camera-axis depth, what cnerf_mesh_raster_visibility writes) or sqrtf((d0 d0 + d1 d1) + d2 d2)
 *         (depth_kind 1: distance along the ray, what a renderer returns)
 *     12. sdf = D - r; skip if sdf < -trunc: the point is hidden behind the surface and this view says nothing about it
 *     13. s = -fminf(1, sdf / trunc): positive inside like a density, -1 in free space, so that marching cubes (inside: value >= level)
 *         winds the faces outwards at level 0
 *     14. acc += w s (the product rounded, then the sum); weight += w
 *   The views go to the device in launches of at most 16, the cameras by value; a point's sums run in view order within and across
 *   launches and calls, so the state does not depend on how the views are cut: n_views = 33 at once, 33 calls of one and 16 + 17 give the
 *   same bytes.  depth / pixel_weight: device float32 [n_views][H][W]; pixel_weight may be NULL.
 *   finalize : volume[i] = weight[i] > 0 ? acc[i] / weight[i] : fill (device float32 [n]); observed (device uint32 [1]) = the number of
 *              points with weight > 0 (an integer count: any order of arrival gives the same value).
 *   face_keep: keep[f] (device uint8 [F]) = 1 when the lattice cell that holds face f's centroid has eight corners with weight > 0, else 0:
 *              c_b = ((v0_b + v1_b) + v2_b) / 3, q_b = clamp(floorf((c_b - org_b) / sp_b), 0, n_b - 2) (NaN -> 0), the cell's corners are
 *              q + {0, 1}^3.  A face with an index outside [0, V) gets 0.  It removes the shell where "behind the surface" meets "never
 *              observed" from the zero-level mesh of finalize's volume.
 *   CNERF_EINVAL: a lattice extent < 2 or more than 2^31 points; (integrate) trunc not finite or <= 0, fx or fy zero or non-finite, cx / cy /
 *   near non-finite, convention or depth_kind outside {0, 1}, H W >= 2^31; (face_keep) V or F >= 2^31.  Then n_views == 0 / F == 0:
 *   CNERF_OK without a launch.  Then CNERF_ENULL: a NULL state, depth, c2w_host, origin_host, spacing_host, volume, observed, faces, keep,
 *   or verts with V > 0.  All return before any launch.  No workspace; no float atomics: the output is bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_tsdf_integrate(float *state, uint32_t nx, uint32_t ny, uint32_t nz, const float *origin_host, const float *spacing_host, float trunc,
                         const float *depth, const float *pixel_weight, uint32_t n_views, uint32_t H, uint32_t W, const float *c2w_host,
                         float fx, float fy, float cx, float cy, int convention, float near, int depth_kind, void *stream);
int cnerf_tsdf_finalize(const float *state, uint32_t nx, uint32_t ny, uint32_t nz, float fill, float *volume, uint32_t *observed, void *stream);
int cnerf_tsdf_face_keep(const float *state, uint32_t nx, uint32_t ny, uint32_t nz, const float *origin_host, const float *spacing_host,
                         const float *verts, uint32_t V, const int32_t *faces, uint32_t F, uint8_t *keep, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-view colour fusion: the colour of surface points (the texels of a bake, the vertices of a mesh) blended from the rendered views
 * that see them (customnerf_amd/mesh.py ViewColors; csrc/mesh_view_colors.hip; the reference has none — NeRF-to-mesh exporters project
 * their renders onto the surface on the host).  All float arithmetic is float32, one rounding per written operation, in the order
 * written (the build has -ffp-contract=off); divisions and square roots are correctly rounded: the rasteriser's rules above.
 *   Points: points / normals device float32 [M][3], p and its unit normal n (not normalised here), in any order; M < 2^31.
 *   Views: images device float32 [n_views][H][W][3], depth device float32 [n_views][H][W] — the depth of THE SURFACE THE POINTS LIE ON
 *   from each camera (cnerf_mesh_raster_visibility: camera-axis depth, depth_kind 0; or a distance along the ray, depth_kind 1) —
 *   pixel_weight device float32 [n_views][H][W] or NULL.  Cameras: those of cnerf_tsdf_integrate, one c2w_host float32 [3][4] per view
 *   on the host, shared fx, fy, cx, cy, convention and near; the vertex transform is the rasteriser's own code (csrc/mesh_camera.h).
 *   State: float32 [M][4] on the device, 16-byte aligned: (sum of w r, sum of w g, sum of w b, sum of w) over the views so far, and seen
 *   uint32 [M], the number of views that added to the point; all zero at first (the caller clears them).
 *   accumulate, per point, for each view v in index order ("skip": this view adds nothing to this point):
 *      1. d = p - t; c_k = (m[0][k] d0 + m[1][k] d1) + m[2][k] d2; z = -c_2 (convention 0) or c_2 (convention 1); skip unless z >= near
 *         (a NaN z fails the test); X = cx + fx (c_0 / z); Y = cy + (-1) (fy (c_1 / z)) (convention 0) or cy + fy (c_1 / z)
 *         (convention 1): steps 1-6 of cnerf_tsdf_integrate
 *      2. pixels are sampled at their centres: u = X - 0.5, v = Y - 0.5, x0 = floorf(u), y0 = floorf(v), ax = u - x0, ay = v - y0; skip
 *         unless the whole 2 x 2 footprint lies in the image: 0 <= x0 <= (float)(W - 2) and 0 <= y0 <= (float)(H - 2), tested on the
 *         floats (non-finite values fail), then (int) x0 + 1 < W and (int) y0 + 1 < H (which can fail only where the float rounds up,
 *         W > 2^24).  A point that projects into the half-pixel border of the image is skipped
 *      3. len = sqrtf((d0 d0 + d1 d1) + d2 d2); r = z (depth_kind 0) or len (depth_kind 1); skip unless ALL FOUR footprint depths
 *         D = depth[v][y0 + j][x0 + i] satisfy D > 0, D < inf and fabsf(D - r) <= depth_tol (NaN fails).  Conservative at silhouettes on
 *         purpose — a footprint that straddles an occluding edge or the background is dropped whole, another view covers that point —
 *         so background never bleeds in
 *      4. cos = -((n0 d0 + n1 d1) + n2 d2) / len; skip unless cos > min_cos; w = cos, then power - 1 times w = w cos (power 1..8).  With
 *         pixel_weight: w = w q, q the bilinear value of the four weights as in 5.  Skip unless 0 < w < inf
 *      5. per channel, with gx = 1 - ax, gy = 1 - ay and c_ij = images[v][y0 + j][x0 + i]:
 *         c = (c00 gx + c10 ax) gy + (c01 gx + c11 ax) ay
 *      6. acc_k += w c_k (the product rounded, then the sum) for k = r, g, b; wsum += w; seen += 1
 *   One launch takes at most 16 views, the cameras by value; n_views > 16 is CNERF_EINVAL and the caller cuts the views.  A point's sums
 *   run in view order within and across launches and calls, so the state does not depend on the cut: 33 views as 16 + 16 + 1, as
 *   1 + 32 or one by one give the same bytes.  Colour and pixel weight are read only where the depth test passed.
 *   resolve: out[i] (device float32 [M][3]) = acc / wsum per channel where wsum > 0, else fallback[i] (device float32 [M][3]) when
 *            fallback != NULL, else fill_host (float32 [3] on the host).  counts (device uint64 [3]) += the number of points with seen
 *            == 0, == 1 and >= 2: resolve adds to what counts holds (the caller clears it), integer adds, so any order of arrival gives
 *            the same value.
 *   CNERF_EINVAL: M >= 2^31; (accumulate) n_views > 16, fx or fy zero or non-finite, cx / cy / near non-finite, convention or depth_kind
 *   outside {0, 1}, depth_tol not finite or <= 0, min_cos outside [0, 1), power outside 1..8, H W >= 2^31.  Then M == 0 or n_views == 0:
 *   CNERF_OK without a launch.  Then CNERF_ENULL: a NULL points, normals, images, depth, c2w_host, state, seen, fill_host, out or
 *   counts; then CNERF_EINVAL for a state that is not 16-byte aligned.  H < 2 or W < 2: CNERF_OK without a launch (no footprint fits).
 *   All return before any launch.  No workspace; no float atomics: the output is bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_view_colors_accumulate(const float *points, const float *normals, uint32_t M, const float *images, const float *depth,
                                 const float *pixel_weight, uint32_t n_views, uint32_t H, uint32_t W, const float *c2w_host, float fx, float fy,
                                 float cx, float cy, int convention, float near, int depth_kind, float depth_tol, float min_cos, int power,
                                 float *state, uint32_t *seen, void *stream);
int cnerf_view_colors_resolve(const float *state, const uint32_t *seen, uint32_t M, const float *fallback, const float *fill_host, float *out,
                              uint64_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Topology report and hole filling (customnerf_amd/mesh.py topology / fill_holes; csrc/mesh_holes.hip; the reference has none).  verts
 * float32 [V][3], optional normals float32 [V][3] (NULL: none), faces int32 [F][3].  V < 2^31 and F <= 0x2AAAAAAA (half-edge ids 3 f + k
 * and loop lengths stay below 2^31), else CNERF_EINVAL; F = 0 returns CNERF_OK without a launch and writes nothing; ws 16-byte aligned and
 * >= workspace_bytes, else CNERF_EINVAL.  The caller's stream and workspace; no allocation, no host sync; the counts are the one host read.
 * The output does not depend on scheduling: integer atomics only, compaction by scan, lists sorted.  flags bit 0: some face index lies
 * outside [0, V), and nothing else is then counted or written.
 *   Definitions: half-edge 3 f + k runs from a = f[k] to b = f[(k + 1) % 3]; with a == b (a face repeating an index) it is no edge.  For
 *   an undirected edge {a, b}, same and opp count the half-edges a -> b and b -> a.  Interior: one of each.  Boundary: one in all.  Every
 *   other edge is non-manifold (more than two faces, or two that use it in one direction).  A boundary half-edge is the half-edge of a
 *   boundary edge.  A vertex is pinched when more than one boundary half-edge leaves it, or more than one ends in it.  Boundary loops
 *   are the connected components of the graph of boundary edges; a loop's label is the smallest half-edge id on it.  A loop is simple
 *   when it holds no pinched vertex and no end of a non-manifold edge: a cycle, and next(a -> b) is the one boundary half-edge leaving b.
 *   topology       : counts (device uint32 [10]) = vertices in a face, undirected edges, boundary edges, non-manifold edges, pinched
 *                    vertices, boundary loops, simple loops, components (vertices joined by a face, as cnerf_mesh_components_*; those
 *                    that hold a face), faces repeating an index, flags.  Any triangle mesh.
 *   topology_loops : after topology on the same stream with the same ws, V and F: loop_lengths [max_loops] int32, the edges of every
 *                    loop in increasing label; entries at or past max_loops are not written.
 *   holes_count    : the mesh must be edge-manifold and consistently oriented with no face repeating an index — flags bit 1: a
 *                    non-manifold edge, bit 2: a face repeating an index; after a flag the counts are 0 and emit writes nothing.
 *                    max_edges: 0 for no limit, else >= 3 (1 and 2: CNERF_EINVAL).  A simple loop of 3 <= n <= max_edges edges is
 *                    filled, every other loop is left open.  counts (device uint32 [6]) = new vertices, new faces, loops filled, loops
 *                    left open as not simple, loops left open as too long, flags.
 *   holes_emit     : after holes_count on the same stream with the same ws and arguments.  verts_out [V + new vertices][3], faces_out
 *                    [F + new faces][3], normals_out (written when normals != NULL): the input is their prefix, bit for bit (vertices
 *                    no face references included).  Then, per filled loop in increasing label: n = 3, a -> b -> c -> a from the label:
 *                    the face (b, a, c), no vertex.  n > 3: one vertex c and, in loop order from the label, the face (b, a, c) for
 *                    every half-edge a -> b — the winding of that half-edge's missing twin.  c = the sum of the loop's positions
 *                    (the a of every half-edge) in fp64 in loop order, divided by n, rounded once to float32.  Its normal: the sum over
 *                    the fan's faces, in loop order, of (p1 - p0) x (p2 - p0) in fp64 from the float32 positions (c as rounded), m;
 *                    l = sqrt((mx mx + my my) + mz mz); (float)(m / l) when l > 0, else 0.  One rounding per written operation, nothing
 *                    fused; division and square root are correctly rounded.  Entries at or past max_verts / max_faces are not written
 *                    (a loop whose fan would cross either is not written at all).
 *   workspace_bytes : about 17 bytes per vertex + 51 per face + 36 per 256 of max(V, 3 F).
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_holes_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_topology(const int32_t *faces, uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts, void *stream);
int cnerf_mesh_topology_loops(uint32_t V, uint32_t F, void *ws, uint64_t ws_bytes, int32_t *loop_lengths, uint32_t max_loops, void *stream);
int cnerf_mesh_holes_count(const int32_t *faces, uint32_t V, uint32_t F, uint32_t max_edges, void *ws, uint64_t ws_bytes, uint32_t *counts,
                           void *stream);
int cnerf_mesh_holes_emit(const float *verts, const float *normals, uint32_t V, const int32_t *faces, uint32_t F, uint32_t max_edges,
                          void *ws, uint64_t ws_bytes, float *verts_out, float *normals_out, int32_t *faces_out, uint32_t max_verts,
                          uint32_t max_faces, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Closest-point queries against a triangle mesh and a deterministic surface sampler: what the deviation report is made of
 * (customnerf_amd/mesh.py build_bvh / closest_point / sample_surface / distance; csrc/mesh_bvh.hip; the reference has none).  verts float32
 * [V][3], faces int32 [F][3].  All arithmetic is float32, one rounding per written operation in the order written (the build has
 * -ffp-contract=off); divisions and square roots are correctly rounded; dot(u, v) = (ux vx + uy vy) + uz vz.
 *   Taking part: a face takes part when its three indices lie in [0, V) and its nine coordinates are finite.  Every other face is left out
 *   of the tree and of the sampler; flags bit 0 = some index lies outside [0, V), bit 1 = some face with valid indices has a non-finite
 *   coordinate.  Neither is an error here: the caller decides.
 *   build   : counts (device uint32 [2]): [0] the faces in the tree, [1] the flags; the one host read.  The faces are ordered along a Morton
 *             curve of their centroids by a radix sort without atomics, so ws is bit-identical from run to run.  ws: 256-byte header |
 *             triangle records (48 B each, in sorted order) | node boxes (32 B each) | sort scratch; a query reads the first three only, needs
 *             neither verts nor faces, and may run any number of times.  The tree's shape is not part of the contract: no output depends on it.
 *   closest : after build with the same ws, V and F.  points float32 [Q][3].  Per query p, over the faces that take part:
 *             dist2 [Q] = the smallest d2(p, face), face [Q] = the smallest face index attaining it, point [Q][3] and bary [Q][3] (either
 *             may be NULL) that face's closest point and its barycentrics (point = b0 v0 + b1 v1 + b2 v2 up to rounding).  A face whose d2
 *             is NaN never wins (every comparison with it is false); +inf may win.  A non-finite p, a tree without faces, or no winner:
 *             face = -1, dist2 = +inf, point = bary = 0.  stats (NULL or device uint64 [2], ADDED to, so zero it first): node boxes tested
 *             and triangles tested, summed over the call.
 *             d2(p, (a, b, c)) — Ericson, Real-Time Collision Detection, 5.1.5; the first region that holds, in this order:
 *               ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c; d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp),
 *               d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
 *               1 vertex a : d1 <= 0 and d2 <= 0                          x = a, bary (1, 0, 0)
 *               2 vertex b : d3 >= 0 and d4 <= d3                         x = b, bary (0, 1, 0)
 *               3 edge ab  : vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3), x = a + v ab, bary (1 - v, v, 0)
 *               4 vertex c : d6 >= 0 and d5 <= d6                         x = c, bary (0, 0, 1)
 *               5 edge ac  : vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6), x = a + w ac, bary (1 - w, 0, w)
 *               6 edge bc  : va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), x = b + w (c - b),
 *                                                                         bary (0, 1 - w, w)
 *               7 inside   : otherwise                                    e = 1 / ((va + vb) + vc), v = vb e, w = vc e,
 *                                                                         x = (a + ab v) + ac w, bary ((1 - v) - w, v, w)
 *               then r = p - x and d2 = (rx rx + ry ry) + rz rz from the rounded x.  (A face with a == b can give 0 / 0 in region 3: NaN.)
 *   sample  : face f that takes part has e1 = v1 - v0, e2 = v2 - v0, c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 *             area A = 0.5 sqrt((cx cx + cy cy) + cz cz) and order k = ceil(sqrt(2 A) / spacing) clamped to [1, 256] (k = 1 when that is
 *             NaN or below 1; a value above 256 sets flags bit 2).  Its k^2 samples are the centroids of the k^2 congruent sub-triangles, in
 *             the order m = 0 .. k^2 - 1: row i = k - ceil(sqrt(k^2 - m)) starts at m = i (2 k - i); rem = m - i (2 k - i), j = rem / 2,
 *             up = rem % 2 (0: the sub-triangle with corners (i, j), (i + 1, j), (i, j + 1) of the k-fold lattice, 1: the inverted one
 *             beside it); u = (float) (3 i + 1 + up) / (float) (3 k), v = (float) (3 j + 1 + up) / (float) (3 k), bary = ((1 - u) - v, u, v),
 *             point = (v0 + u e1) + v e2 per component (exact in a coordinate the three vertices share), weight = A / (float) (k k).  A
 *             zero-area face gives one sample of weight 0.
 *             Samples come in face order; outputs points [n][3], face int32 [n], bary [n][3], weight [n].
 *             count : counts (device uint64 [2]): [0] the number of samples n, exact, [1] the flags; the one host read.
 *             emit  : after count on the same stream with the same ws and arguments; writes the samples with index < max_samples.  When
 *                     n >= 2^32 it writes nothing.
 *   CNERF_ENULL: a required pointer is NULL.  CNERF_EINVAL: V, F or Q >= 2^31, a short or misaligned (16 bytes) ws, spacing not finite or
 *   <= 0.  Both return before any launch; F = 0 and Q = 0 are accepted.  The caller's stream and workspace; no allocation, no host sync,
 *   no float atomics; the integer atomics (flags, the count, the centroid box as integer maxima, stats) do not depend on their order, so
 *   every output is bit-reproducible.  bvh workspace_bytes: 48 (records) + 16 (sort keys) + 16 .. 32 (boxes) bytes per face; sample workspace_bytes: 256 + F / 32.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_bvh_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_bvh_build(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, void *ws, uint64_t ws_bytes, uint32_t *counts,
                         void *stream);
int cnerf_mesh_bvh_closest(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *points, uint32_t Q, float *dist2,
                           int32_t *face, float *point, float *bary, uint64_t *stats, void *stream);
int cnerf_mesh_sample_workspace_bytes(uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_sample_count(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, float spacing, void *ws, uint64_t ws_bytes,
                            uint64_t *counts, void *stream);
int cnerf_mesh_sample_emit(const float *verts, uint32_t V, const int32_t *faces, uint32_t F, float spacing, void *ws, uint64_t ws_bytes,
                           float *points, int32_t *face, float *bary, float *weight, uint64_t max_samples, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Ray queries against the tree of cnerf_mesh_bvh_build: the closest hit and the any-hit bit (customnerf_amd/mesh.py ray_cast / occluded /
 * ambient_occlusion; csrc/mesh_bvh.hip; the reference has none).  After build with the same ws, V and F; the faces that take part are
 * those of the build.  origins, dirs float32 [Q][3]; the direction is not normalised and t is in units of |d|.  float32, one rounding per
 * written operation in the order written, divisions correctly rounded, exactly as above; tests/ray_restatement.py restates the rule.
 *   The ray/triangle rule is the watertight test of Woop, Benthin and Wald (JCGT 2(1), 2013): a ray through an edge or a vertex that two
 *   faces share hits at least one of them, because both evaluate the shared edge's function from the same two sheared points, with the
 *   opposite sign and the same magnitude, and a zero is settled exactly.
 *   Per ray (o, d): kz = the axis of the largest |d| (the lowest axis on a tie); kx = (kz + 1) mod 3, ky = (kx + 1) mod 3, the two swapped
 *     when d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 *   Per face (a, b, c): A = a - o per component (B, C alike); Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz] (B, C alike);
 *     U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.  When U, V or W is exactly 0, all three are computed again in float64 from the
 *     float32 Ax .. Cy (the products are then exact), the signs are taken from the float64 values, and U, V, W become their float32
 *     roundings.  A miss when some of the three is < 0 and some is > 0.  det = (U + V) + W; a miss when det == 0; cull 1 (back) misses
 *     when det < 0, cull 2 (front) when det > 0 (det > 0: the ray meets the side (b - a) x (c - a) points to, the front of a face wound
 *     outwards — the convention of cnerf_mesh_raster_visibility).  Az = Sz A[kz] (Bz, Cz alike), t = ((U Az + V Bz) + W Cz) / det,
 *     bary = (U / det, V / det, W / det).  The face is hit when t_min <= t <= t_max (false for a NaN).
 *   raycast : t_out [Q] = the smallest t over the faces hit, face_out [Q] = the smallest face index attaining it, bary_out [Q][3] that face's
 *     barycentrics (a miss: t = +inf, face = -1, bary = 0).  Any of the three may be NULL.
 *   occluded : occluded [Q] uint8 = 1 when some face is hit, else 0.
 *   The range is t_min / t_max for every ray, or t_min_per_ray[q] / t_max_per_ray[q] where that pointer is not NULL.
 *   A ray misses everything when a component of o or d is not finite, d = 0, Sx, Sy or Sz is not finite, or t_min > t_max.
 *   stats (NULL or device uint64 [2], ADDED to, so zero it first): node boxes tested and triangles tested, summed over the call.  The tree
 *   only prunes: every output is the brute-force result over the faces, bit for bit (csrc/mesh_bvh.hip says why, for coordinates whose
 *   products do not overflow).
 *   CNERF_ENULL: a required pointer is NULL.  CNERF_EINVAL: V, F or Q >= 2^31, a short or misaligned ws, cull outside 0 .. 2.  Both return
 *   before any launch; Q = 0 is accepted.  The caller's stream; no allocation, no host sync; the only atomics are the integer stats.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_bvh_raycast(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *origins, const float *dirs, uint32_t Q,
                           float t_min, float t_max, const float *t_min_per_ray, const float *t_max_per_ray, int cull, float *t_out,
                           int32_t *face_out, float *bary_out, uint64_t *stats, void *stream);
int cnerf_mesh_bvh_occluded(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const float *origins, const float *dirs, uint32_t Q,
                            float t_min, float t_max, const float *t_min_per_ray, const float *t_max_per_ray, int cull, uint8_t *occluded,
                            uint64_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Projection of points onto a source mesh along a direction, within a reach: what a texture baker moves the texels of a low-polygon mesh
 * onto the high-resolution surface with (customnerf_amd/mesh.py project_to_surface / bake_texture(source=); csrc/mesh_bvh.hip,
 * k_bvh_project; the reference has none).  After build over the SOURCE mesh with the same ws, V and F; faces int32 [F][3] are the source's
 * (read for the normals' indices only: the positions are the tree's records), normals float32 [V][3] the source's vertex normals or NULL.
 * x float32 [Q][3] the points, n float32 [Q][3] their directions (the low mesh's outward normal, not normalised: offsets are in units of
 * |n|), reach for every query or reach_per_query[q] where that pointer is not NULL.  float32, one rounding per written operation in the
 * order written, divisions and square roots correctly rounded, exactly as above; tests/project_restatement.py restates the rule.
 *   Per query, the two rays and then the closest point:
 *     forward  : the raycast rule for origin x, direction n, range [0, reach], cull 2 -> t_f, face, barycentrics.  Along +n only faces
 *                whose front looks the way n does are accepted, and those are met from behind.
 *     backward : the raycast rule for origin x, direction (-n0, -n1, -n2), range [0, reach], cull 1 -> t_b, face, barycentrics.
 *                (The culls keep a point of a thin part from landing on the opposite wall, whose faces look the other way.)
 *     kind 2 when the backward ray hit and either the forward ray missed or t_b < t_f: that hit, offset = -t_b.
 *     kind 1 otherwise, when the forward ray hit (a tie goes forward): that hit, offset = t_f.
 *     kind 3 when both missed and the closest rule of cnerf_mesh_bvh_closest for x finds a face with
 *            dist2 <= (reach reach) ((n0 n0 + n1 n1) + n2 n2): that face, its closest point cp and barycentrics;
 *            r = cp - x, offset = ((r0 n0 + r1 n1) + r2 n2) / ((n0 n0 + n1 n1) + n2 n2).
 *     kind 0 otherwise, and for a degenerate query: a component of x or n not finite, n = 0, a reach that is negative or NaN, or a tree
 *            without faces.  (A direction the raycast rule calls degenerate although it is finite and not 0 misses with both rays and
 *            goes on to the closest rule.)
 *   point [Q][3] : kinds 1, 2: (b0 a + b1 b) + b2 c per component, a, b, c the hit face's float32 vertices and b its barycentrics by the
 *                  raycast rule; kind 3: cp; kind 0: x, bit for bit.
 *   normal [Q][3]: unit(v) = v / sqrt((v0 v0 + v1 v1) + v2 v2), defined when that sum is positive and finite (the rule of the atlas's view
 *                  direction without its sign).  Kinds 1 - 3, with normals: unit((b0 n_a + b1 n_b) + b2 n_c) of the face's three vertex
 *                  normals; where that is not defined, or normals is NULL: unit(e1 x e2) with e1 = b - a, e2 = c - a,
 *                  e1 x e2 = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); where that is not defined, and for kind 0: unit(n);
 *                  where that is not defined: (0, 0, 1).
 *   offset [Q]   : as above, the signed distance from x to point along n in units of |n|; 0 for kind 0.
 *   face [Q] int32 : the source face, -1 for kind 0.   kind [Q] uint8 : 0 .. 3.
 *   Any of the five may be NULL.  stats (NULL or device uint64 [2], ADDED to, so zero it first): node boxes tested and triangles tested,
 *   summed over the call.  The second ray is walked over [0, min(reach, t_f)] — by the strict t_b < t_f no result depends on that — and
 *   the closest point is searched only by the queries both rays left without a face, so one call tests no more than the two raycast
 *   calls (and, where needed, the closest call) it stands for.
 *   CNERF_ENULL: ws, x, n or (with F > 0) faces is NULL.  CNERF_EINVAL: V, F or Q >= 2^31, a short or misaligned ws, a reach that is
 *   negative or NaN where reach_per_query is NULL.  Both return before any launch; Q = 0 is accepted.  The caller's stream; no allocation,
 *   no host sync; the only atomics are the integer stats; every output is the brute-force result over the faces, bit for bit.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_bvh_project(const void *ws, uint64_t ws_bytes, uint32_t V, uint32_t F, const int32_t *faces, const float *normals,
                           const float *x, const float *n, uint32_t Q, float reach, const float *reach_per_query, float *point,
                           float *normal, float *offset, int32_t *face, uint8_t *kind, uint64_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Inside or outside: the generalized winding number of a point about the faces of the tree of cnerf_mesh_bvh_build, and the signed
 * distance made of it and the closest-point rule (customnerf_amd/mesh.py winding_number / contains / signed_distance / voxel_remesh;
 * csrc/mesh_bvh.hip; the reference has none).  The winding number tolerates holes, self-intersections and non-manifold edges (Jacobson,
 * Kavan and Sorkine-Hornung 2013); far parts of the mesh are taken whole through the first (dipole) term of the expansion of Barill,
 * Dym, Kazhdan, Schneider and Jacobson 2018, kept per tree node in a buffer of its own: bvh_ws is read only, its layout and
 * cnerf_mesh_bvh_workspace_bytes are what they were.  float32, one rounding per written operation in the order written, divisions and
 * square roots correctly rounded, dot(u, v) = (ux vx + uy vy) + uz vz, exactly as above; cross(u, v) = (uy vz - uz vy, uz vx - ux vz,
 * ux vy - uy vx), len(u) = sqrt(dot(u, u)); tests/winding_restatement.py restates the rules.  Unlike the results above, these DO depend on
 * the tree: its shape is the one the build gives — the records in sorted order, BV_LEAF = 4 to a leaf, NL = ceil(n / 4) leaves, depth
 * D = ceil(log2 NL), node (d, j) at heap index 2^d + j covering the leaves [j NL >> d, (j + 1) NL >> d), children 2 i and 2 i + 1.
 *   moments (cnerf_mesh_winding_build, after cnerf_mesh_bvh_build with the same bvh_ws, V and F): mom holds two float4 per heap index i, at
 *     [2 i] = (p.x, p.y, p.z, r) — a centre and the radius of a ball about it that holds the node's vertices — and at [2 i + 1] =
 *     (N.x, N.y, N.z, A) — the sum of the faces' area vectors and of their areas.  Indices 1 .. 2^(D + 1) - 1 are written, nothing else.
 *     leaf (a node of level D), over the valid records of its leaf (at most one leaf, at most four records) in slot order, with the sums
 *       started at 0: e1 = b - a, e2 = c - a, x = cross(e1, e2), A_i = 0.5 len(x), c_i = ((a + b) + c) / 3 per component;
 *       A = A + A_i, N = N + 0.5 x, S = S + A_i c_i, M = M + c_i per component.  Then p = S / A, or M / (float) count when A == 0, per
 *       component, and r = the largest len(v - p) over the records' vertices v, started at 0.
 *     inner node, from the left child (p_l, r_l, N_l, A_l) and the right one: A = A_l + A_r, N = N_l + N_r,
 *       p = (A_l p_l + A_r p_r) / A, or 0.5 (p_l + p_r) when A == 0, per component, r = max(len(p - p_l) + r_l, len(p - p_r) + r_r).
 *     empty node (no valid record below it: the NaN padding, a node of level D that covers no leaf): p = N = 0, A = 0, r = -1.  A node with
 *       an empty left child is a copy of its right child, bit for bit; otherwise one with an empty right child is a copy of its left.
 *   winding (cnerf_mesh_winding_query): per query q, a depth-first walk from the root, the left child before the right, w started at 0:
 *     an empty node (r < 0) is passed over.  With d = p - q per component and d2 = dot(d, d), a node is accepted whole when
 *     d2 > (beta beta) (r r) (false when that product is NaN, as for beta = +inf and r = 0): w = w + dot(N, d) / (FOURPI (d2 sqrt(d2))),
 *     FOURPI = 12.566370614359172f.  Otherwise the walk descends, and at level D each valid record of the leaf, in slot order, adds
 *     the solid angle of Van Oosterom and Strackee 1983: a = A - q, b = B - q, c = C - q per component (A, B, C the record's vertices),
 *     num = dot(a, cross(b, c)); a term of 0 when num == 0; la = len(a), lb = len(b), lc = len(c),
 *     den = (((la lb) lc + dot(a, b) lc) + dot(b, c) la) + dot(c, a) lb, w = w + (2 atan2f(num, den)) / FOURPI.
 *     atan2f is the device library's (a few ulp, not correctly rounded): the one step that is not restated bit for bit.  A mesh wound
 *     outwards — (b - a) x (c - a) points out, the convention of the rasteriser and the ray queries — has w = 1 inside and 0 outside.
 *     beta = +inf accepts nothing: w is the sum over all the faces in tree order.  A non-finite q or a tree without faces: w = 0.
 *     stats (NULL or device uint64 [2], ADDED to, so zero it first): nodes accepted and triangles evaluated, summed over the call.
 *   signed distance (cnerf_mesh_bvh_signed_distance): dist2 and face by the rule of cnerf_mesh_bvh_closest, unchanged, w as above (stored
 *     when winding is not NULL); signed_dist [Q] = -sqrt(dist2) when w >= 0.5, else sqrt(dist2): negative inside.  A non-finite q or a tree
 *     without faces: signed_dist = +inf, face = -1, w = 0.  stats as for the winding query.
 *   CNERF_ENULL: a required pointer (bvh_ws, mom; with Q > 0 points and winding, or signed_dist and face) is NULL.  CNERF_EINVAL: V, F or
 *   Q >= 2^31, a short or misaligned (16 bytes) bvh_ws or mom, beta < 1 or NaN.  Both return before any launch; Q = 0 is accepted.  The
 *   caller's stream and buffers; no allocation, no host sync, no float atomics: a query's terms add up in the order of its own walk, so
 *   every output is bit-reproducible.  workspace_bytes: 32 bytes per heap index, 32 * 2^(Dmax + 1) with Dmax the depth of a tree of F faces.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_mesh_winding_workspace_bytes(uint32_t V, uint32_t F, uint64_t *bytes_host);
int cnerf_mesh_winding_build(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, void *mom, uint64_t mom_bytes, void *stream);
int cnerf_mesh_winding_query(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, const void *mom, uint64_t mom_bytes,
                             const float *points, uint32_t Q, float beta, float *winding, uint64_t *stats, void *stream);
int cnerf_mesh_bvh_signed_distance(const void *bvh_ws, uint64_t bvh_bytes, uint32_t V, uint32_t F, const void *mom, uint64_t mom_bytes,
                                   const float *points, uint32_t Q, float beta, float *signed_dist, int32_t *face, float *winding,
                                   uint64_t *stats, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Image scores: squared error, absolute error and SSIM between two image batches in one pass (customnerf_amd/metrics.py image_metrics /
 * psnr / ssim, the trainers' evaluate(); csrc/metrics.hip; additive, same ABI version).  The reference scores on the host
 * (utils_init_nerf.py:673-779) and has no SSIM.
 *   pred, target [B][H][W][C] channel-last, float32 or float16 (dtype), C in {1, 3}: the layout eval_step / test_step return.
 *   mask NULL or float32 [B][H][W]: a pixel counts when its mask value is nonzero.
 *   quantize != 0: both images first go through q(v) = floor(clamp(v, 0, 1) * 255) / 255, evaluated in float32 (float16 input is widened
 *     first): the value an 8-bit file written by truncation holds (`(pred * 255).astype(np.uint8)`, utils_init_nerf.py:550, plus a clamp).
 *   sums_out [B][5] float64 (device), per image:
 *     [0] sum of (a - b)^2 and [1] sum of |a - b| over the counted pixels and all channels, [2] the number of counted pixel-channels,
 *     [3] the sum of the SSIM map over the counted windows and all channels, [4] the number of counted window-channels.
 *     mse = [0] / [2], l1 = [1] / [2], psnr = 10 log10(1 / mse), ssim = [3] / [4] are the caller's, in float64.  An image without counted
 *     pixels has [2] = 0 (0 / 0 = nan there): a defined result, not an error.
 *   SSIM, because libraries differ: Wang, Bovik, Sheikh and Simoncelli 2004 with L = 1, K1 = 0.01, K2 = 0.03 (C1 = K1 K1, C2 = K2 K2); an
 *     11-tap Gaussian window of sigma 1.5, g[k] = exp(-(k - 5)^2 / 4.5) computed in float64 and divided by its sum, applied separably
 *     (rows first) over the valid region only — the map is (H - 10) x (W - 10) per channel, no padding; population moments
 *     mu_a = E[a], var_a = E[a a] - mu_a mu_a, cov = E[a b] - mu_a mu_b under that window;
 *     map = ((2 mu_a mu_b + C1) (2 cov + C2)) / ((mu_a mu_a + mu_b mu_b + C1) (var_a + var_b + C2)), per channel.
 *     Window (y, x) of the map covers pixels [y, y + 10] x [x, x + 10]; with a mask it counts when its centre pixel (y + 5, x + 5) does.
 *     An image's SSIM is the mean of the map over the counted windows and the channels.
 *   Numerics: the inputs convert to float64 exactly; the five window moments, the SSIM expression and every sum are float64 (float32
 *     moments lose 1e-4 of SSIM on flat images: DESIGN.md section 4d).  Identical images give a map of exactly 1.  Partial sums are one per
 *     32 x 32 tile of one (image, channel), added in a fixed order: no atomics, bit-reproducible from run to run.
 *   ssim_map NULL or float32 [B][H - 10][W - 10][C]: the whole map, rounded to float32, whatever the mask says.
 *   workspace: cnerf_image_metrics_workspace_bytes(B, H, W, C) bytes, 8-byte aligned, contents irrelevant.
 *   CNERF_EINVAL: C not 1 or 3, H or W below 11 or above 65535, B C above 65535, an unknown dtype, a misaligned workspace or sums_out.
 *   CNERF_ENULL: pred, target, sums_out or workspace NULL (bytes_host for the query).  Both return before any launch; B = 0 is accepted
 *   without one.  The caller's stream and buffers, no allocation, no host sync.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_image_metrics_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint64_t *bytes_host);
int cnerf_image_metrics(const void *pred, const void *target, const float *mask, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int dtype,
                        int quantize, double *sums_out, float *ssim_map, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The gradient of an image's SSIM with respect to pred (customnerf_amd/metrics.py ssim_with_grad / ssim_loss, the trainers'
 * opt.lambda_dssim; csrc/metrics.hip; additive, same ABI version).  The definition of SSIM, the layouts of pred / target / mask, the dtypes
 * and the counting rule are those of cnerf_image_metrics above, with quantize = 0.
 *   sums_out [B][5] float64 (device): the five sums of cnerf_image_metrics, bit for bit (one device routine forms both).
 *   grad_unit [B][H][W][C] float32 (device): d ssim_b / d pred, ssim_b = sums_out[b][3] / sums_out[b][4].
 *   Per channel plane, a = pred, b = target, <.> the windowed mean, per window p:
 *     mu_a = <a>, mu_b = <b>
 *     A1 = 2 mu_a mu_b + C1                   A2 = 2 (<ab> - mu_a mu_b) + C2
 *     B1 = mu_a mu_a + mu_b mu_b + C1         B2 = (<aa> - mu_a mu_a) + (<bb> - mu_b mu_b) + C2          s = A1 A2 / (B1 B2)
 *     d_ab = 2 A1 / (B1 B2)       d_aa = -s / B2       d_mu = 2 mu_b (A2 - A1) / (B1 B2) + 2 mu_a s (1 / B2 - 1 / B1)
 *   (d_ab = ds / d<ab>, d_aa = ds / d<aa>, d_mu = ds / d mu_a with the second moments held).  With the weight g_p = 1 / sums_out[b][4] for
 *   a counted window and 0 for any other, and Wt the TRANSPOSED window filter, Wt[m](y, x) = sum_k sum_l g[k] g[l] m(y - k, x - l) with m zero
 *   outside the (H - 10) x (W - 10) map, the gradient at pixel q is
 *     grad_unit_q = Wt[g d_mu]_q + 2 a_q Wt[g d_aa]_q + b_q Wt[g d_ab]_q.
 *   An image without a counted window gets a plane of exact zeros (never NaN); its sums_out is what cnerf_image_metrics reports.
 *   Numerics: moments, coefficient maps and the transposed filter are float64; each gradient element is rounded to float32 once, after the
 *     division by the window count.  A gather (one thread per pixel reads the maps), no atomics: bit-reproducible from run to run.
 *   Launches: coefficient maps + tile partials, the partial sum, the gather — which reads the window count from sums_out on the device, so
 *     there is no host sync and the call can be captured in a graph.
 *   workspace: cnerf_ssim_grad_workspace_bytes(B, H, W, C) bytes (the tile partials and three float64 maps [B C][3][H - 10][W - 10]),
 *     8-byte aligned, contents irrelevant.
 *   CNERF_EINVAL / CNERF_ENULL as for cnerf_image_metrics (grad_unit is required too); both return before any launch; B = 0 is accepted
 *   without one.  The caller's stream and buffers, no allocation.
 * ---------------------------------------------------------------------------------------------- */
int cnerf_ssim_grad_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint64_t *bytes_host);
int cnerf_ssim_grad(const void *pred, const void *target, const float *mask, uint32_t B, uint32_t H, uint32_t W, uint32_t C, int dtype,
                    double *sums_out, float *grad_unit, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CUSTOMNERF_HIP_H */
