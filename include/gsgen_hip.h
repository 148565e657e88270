/*
 * gsgen_hip.h -- C ABI of libgsgen_hip.so, the MI355X (gfx950) rasterizer behind GSGEN's
 * `_gs` extension.
 *
 * The reference binds this path through a pybind11/torch module (`gs/src/bindings.cpp:5-82`,
 * prototypes `gs/src/render.h:3-155`) whose wrappers (`gs/src/render.cu`) unpack tensors to
 * raw pointers and call `*_cuda(...)` launchers.  The entry points below are those launchers'
 * replacement: plain pointers + sizes + a hipStream_t, no torch types.  All pointers are DEVICE
 * pointers unless stated.  Every function returns 0 on success, a positive hipError_t value
 * when a HIP call failed, or a negative GSGEN_E* code for a violated precondition; nothing
 * calls exit() (the reference's cudaCheck does: gs/src/include/common.h:56-72).
 *
 * Ownership follows the reference: the caller allocates every array, outputs
 * included, and pre-initialises them as the reference's Python does (out = 0, T = 1,
 * start/end = -1, grad_* = 0 -- the backward entry points ACCUMULATE into grad_*).
 * All work is enqueued on `stream`; no entry point synchronises the device or allocates.
 *
 * Layouts (row-major, fp32 unless noted): mean2d [N,2]; cov2d [N,2,2]; color [N,3];
 * alpha [N]; scalar [N]; sh_coeffs [N,3,C*C]; start/end int32 [n_tiles_h*n_tiles_w];
 * gaussian_ids int32 [D]; out [H,W,3] (or [H,W] scalar); T [H,W]; topleft [2]; bg_rgb [3].
 * Alignment of the PARAMETER arrays (mean [N,3], qvec [N,4], svec [N,3], alpha, color, sh_coeffs and their gradients): 4 bytes, the
 * type's own -- they may be views at any float offset into one larger buffer (gsgen_amd.optim.FusedAdam: qvec starts 3 N floats in,
 * svec 7 N, sh_coeffs 11 N, so after a densify they are 16-byte aligned only where N % 4 == 0).  The projection reads mean / qvec /
 * svec element by element; the SH kernels read a row of sh_coeffs (the staging of the exact kernels at C = 2 and 4, the polynomial
 * transform at C = 4) as 16-byte loads from GLOBAL memory, which gfx950 performs at any dword address -- results do not depend on the
 * base's alignment (tests/test_gpu_step_kernels.py renders bit-identical images from both).  The bound passes (gsgen_sh_l1_bound*)
 * take their float4 kernels for a 16-byte aligned base at C = 4 and the row-per-thread kernels otherwise: the same bound within the
 * rounding of the sum's order.  Arrays for which an entry point states 8 or 16 bytes below keep that requirement.
 * tile_size: 16 is the reference's only configured value (conf/base.yaml:132) and the size every tuned kernel variant,
 * the batched, segmented and fused entry points are built for.  The per-camera entry points of the `_gs` surface
 * (gsgen_tile_culling_aabb_count, gsgen_vol_render_start_end_with_T / _backward_start_end, _scalar / _scalar_backward,
 * _sh / _backward_sh) take ANY tile_size from 1 to 32, as the reference's launch of tile_size x tile_size <= 1024 threads does
 * (vol_render.h:1001-1004): 8 runs one wavefront per tile, every other side a four-wavefront workgroup over a 32 x 32 patch of
 * which the caller's tile is the top-left part (untuned: a compatibility path); binning works on tile-index rectangles and is
 * size-agnostic.  tile_size 0 or > 32 returns GSGEN_EUNSUPPORTED.  Per-pixel results do not depend on the tile size.
 */
#ifndef GSGEN_HIP_H
#define GSGEN_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported (the declarations
 * carry default visibility; the cross-file helpers of the implementation stay out of the dynamic symbol table). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef void *gsgen_stream_t; /* hipStream_t; NULL = the legacy default stream */

#define GSGEN_EUNSUPPORTED (-2) /* tile_size not in 1 .. 32 (16 only: batched / segmented / fused), C not in 1..4, kNN K not in 1..32, FPS dim / method, image loss window / channels, depth loss B > 65535, MLP background B H W > 2^31 */
#define GSGEN_EINVAL (-3)       /* null pointer / inconsistent sizes */
#define GSGEN_EWORKSPACE (-4)   /* workspace too small */

const char *gsgen_version(void);
/* HIP error string for positive return codes, own text for negative ones. */
const char *gsgen_error_string(int code);
/* Which compiled kernel variant a compositing launch runs in this process (gsgen_amd/csrc/composite.hip "launch
 * helpers"; the library reads nothing from the environment).  stage: "sh_fwd", "sh_bwd", "sh_fwd_batch", "sh_bwd_batch"
 * (+ "_poly": the polynomial-basis kernel of a bounded enqueue, see gsgen_vol_render_sh_batch_bounded), "rgb_fwd",
 * "rgb_bwd", "rgbd_fwd_batch", "rgbd_bwd_batch".  Writes a NUL-terminated name into out[out_bytes] and returns its
 * length, 0 for an unknown stage.  Host-only; no counterpart in the reference (bench.py reports it next to the measured
 * kernel time). */
int gsgen_kernel_variant(const char *stage, uint32_t C, uint32_t n_segments, char *out, size_t out_bytes);

/* ---- frustum cull ------------------------------------------------------------------
 * replaces culling_gaussian_bsphere, gs/src/render.h:3 -> render.cu:16-44 ->
 * culling_gaussian_bsphere_cuda culling.h:21-33.  mask is bool[N] (1 byte each). */
int gsgen_culling_gaussian_bsphere(uint32_t N, const float *mean, const float *qvec,
                                   const float *svec, const float *normal /*[6,3]*/,
                                   const float *pts /*[6,3]*/, uint8_t *mask, float thresh,
                                   gsgen_stream_t stream);

/* ---- tile binning + per-tile depth sort ---------------------------------------------
 * replaces tile_culling_aabb_start_end, render.h:61 -> render.cu:381-398 ->
 * tile_culling_aabb_start_end_cuda aabb_culling.h:192-260.  D = gaussian_ids length =
 * sum over Gaussians of (br-tl+1) products (the caller's N_with_dub).  Unlike the reference
 * there is no cudaMalloc/cudaFree/blocking memcpy: temporaries live in `workspace`.
 * D (and D_cap of the fused entry points) must not exceed INT32_MAX -- start / end and the list positions are int32 as in
 * the reference -- else GSGEN_EINVAL.  The fused entry points report the frame's pair count in *total; counts that do not
 * fit 32 bits SATURATE at 2^32 - 1 (and read as "does not fit": nothing is binned), they never wrap. */
size_t gsgen_tile_culling_workspace_bytes(uint32_t N, uint32_t D, uint32_t n_tiles);
int gsgen_tile_culling_aabb_start_end(uint32_t N, uint32_t D, uint32_t n_tiles_h,
                                      uint32_t n_tiles_w, const int *aabb_topleft,
                                      const int *aabb_bottomright, const float *depth,
                                      int *gaussian_ids, int *start, int *end, void *workspace,
                                      size_t workspace_bytes, gsgen_stream_t stream);

/* ---- RGB compositing -----------------------------------------------------------------
 * forward with T: tile_based_vol_rendering_start_end_with_T render.h:149 -> render.cu:989-1012
 *   -> ..._cuda_with_T vol_render.h:1064-1078.  T may be NULL (= tile_based_vol_rendering_start_end,
 *   render.h:65 -> vol_render.h:849-864).
 * backward: tile_based_vol_rendering_backward_start_end render.h:73 -> render.cu:426-482 ->
 *   vol_render.h:975-992.  `out` is the saved forward image INCLUDING T*bg. */
int gsgen_vol_render_start_end_with_T(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                      const float *color, const float *alpha, const int *start,
                                      const int *end, const int *gaussian_ids, float *out,
                                      const float *topleft, uint32_t tile_size, uint32_t n_tiles_h,
                                      uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                      uint32_t H, uint32_t W, float thresh, float *T,
                                      gsgen_stream_t stream);
int gsgen_vol_render_backward_start_end(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                        const float *color, const float *alpha, const int *start,
                                        const int *end, const int *gaussian_ids, const float *out,
                                        float *grad_mean, float *grad_cov, float *grad_color,
                                        float *grad_alpha, const float *grad_out,
                                        const float *topleft, uint32_t tile_size,
                                        uint32_t n_tiles_h, uint32_t n_tiles_w, float pixel_size_x,
                                        float pixel_size_y, uint32_t H, uint32_t W, float thresh,
                                        gsgen_stream_t stream);

/* ---- scalar compositing (depth / opacity / z^2 heads) ---------------------------------
 * tile_based_vol_rendering_scalar render.h:131 -> vol_render_scalar.h:47-102;
 * tile_based_vol_rendering_scalar_backward render.h:139 -> vol_render_scalar.h:148-234. */
int gsgen_vol_render_scalar(uint32_t N, uint32_t D, const float *mean, const float *cov,
                            const float *scalar, const float *alpha, const int *start,
                            const int *end, const int *gaussian_ids, float *out,
                            const float *topleft, uint32_t tile_size, uint32_t n_tiles_h,
                            uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                            uint32_t W, float thresh, float *T, gsgen_stream_t stream);
int gsgen_vol_render_scalar_backward(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                     const float *scalar, const float *alpha, const int *start,
                                     const int *end, const int *gaussian_ids, const float *out,
                                     float *grad_mean, float *grad_cov, float *grad_scalar,
                                     float *grad_alpha, const float *grad_out, const float *topleft,
                                     uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w,
                                     float pixel_size_x, float pixel_size_y, uint32_t H, uint32_t W,
                                     float thresh, gsgen_stream_t stream);

/* ---- spherical-harmonic compositing ---------------------------------------------------
 * tile_based_vol_rendering_sh render.h:83 / _sh_with_bg render.h:113 -> vol_render_sh.h:171-265,
 * vol_render_bg.h:12-127;  backward render.h:91 / :121 -> vol_render_sh.h:353-480,
 * vol_render_bg.h:131-265.  `c2w` is read as the reference reads it: 9 consecutive floats =
 * three packed rows (vol_render_sh.h:48-55).  bg_rgb == NULL selects the no-background
 * variant; with bg_rgb the forward adds bg*T and writes bg to empty tiles, and `out` handed to
 * the backward includes it.  T (optional, may be NULL) additionally receives the final
 * transmittance -- an output the reference does not have. */
int gsgen_vol_render_sh(uint32_t N, uint32_t D, const float *mean, const float *cov,
                        const float *sh_coeffs, const float *alpha, const int *start,
                        const int *end, const int *gaussian_ids, float *out, const float *topleft,
                        const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                        uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                        uint32_t W, uint32_t C, float thresh, const float *bg_rgb, float *T,
                        gsgen_stream_t stream);
int gsgen_vol_render_backward_sh(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                 const float *sh_coeffs, const float *alpha, const int *start,
                                 const int *end, const int *gaussian_ids, const float *out,
                                 float *grad_mean, float *grad_cov, float *grad_sh_coeffs,
                                 float *grad_alpha, const float *grad_out, const float *topleft,
                                 const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                 uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                 uint32_t H, uint32_t W, uint32_t C, float thresh,
                                 const float *bg_rgb, gsgen_stream_t stream);

/* ---- additive entry points (no native counterpart in the reference) -------------------
 * EWA projection: the reference does this in PyTorch (gs/renderer.py:366-421); same outputs.
 * c2w is a device pointer to the row-major [3,4] pose.  JW may be NULL.  The backward
 * OVERWRITES g_mean [N,3], g_qvec [N,4], g_svec [N,3]; g_depth may be NULL. */
int gsgen_project_gaussians(uint32_t N, const float *mean, const float *qvec, const float *svec,
                            const float *c2w, float *mean2d, float *cov2d, float *JW, float *depth,
                            gsgen_stream_t stream);
int gsgen_project_gaussians_backward(uint32_t N, const float *mean, const float *qvec,
                                     const float *svec, const float *c2w, int detach_depth,
                                     const float *g_mean2d, const float *g_cov2d,
                                     const float *g_depth, float *g_mean, float *g_qvec,
                                     float *g_svec, gsgen_stream_t stream);
/* Same, rows with mask[i]==0 get zero gradients (mask may be NULL): the backward leg of
 * gsgen_frame_geometry, which keeps every array full-N instead of compacting by the mask. */
int gsgen_project_gaussians_backward_masked(uint32_t N, const float *mean, const float *qvec,
                                            const float *svec, const float *c2w, int detach_depth,
                                            const uint8_t *mask, const float *g_mean2d,
                                            const float *g_cov2d, const float *g_depth,
                                            float *g_mean, float *g_qvec, float *g_svec,
                                            gsgen_stream_t stream);
/* Same, ADDED atomically into caller-zeroed g_mean/g_qvec/g_svec (masked-out rows untouched):
 * the cameras of a batch accumulate into one set of parameter gradients, possibly from
 * concurrent streams. */
int gsgen_project_gaussians_backward_accum(uint32_t N, const float *mean, const float *qvec,
                                           const float *svec, const float *c2w, int detach_depth,
                                           const uint8_t *mask, const float *g_mean2d,
                                           const float *g_cov2d, const float *g_depth,
                                           float *g_mean, float *g_qvec, float *g_svec,
                                           gsgen_stream_t stream);
/* The cameras of a batch in ONE launch: g_* (OVERWRITTEN) = sum over the views of the masked backward
 * above, each Gaussian summed in registers in view order (no atomics, no zero-fill, one pass over the
 * parameters).  c2w / mask / g_mean2d / g_cov2d / g_depth are HOST arrays of n_views DEVICE pointers
 * (read before the call returns); mask and g_depth may be NULL as arrays or per view.  c2w[v] is the
 * row-major [3,4] pose (the first 12 floats of a gsgen_frame_geometry camera block). */
int gsgen_project_gaussians_backward_batch(uint32_t n_views, uint32_t N, const float *mean, const float *qvec,
                                           const float *svec, const float *const *c2w, int detach_depth,
                                           const uint8_t *const *mask, const float *const *g_mean2d,
                                           const float *const *g_cov2d, const float *const *g_depth,
                                           float *g_mean, float *g_qvec, float *g_svec, gsgen_stream_t stream);
/* torch.optim.Adam step (no weight decay, no amsgrad: gs/gaussian_splatting.py:398-419,
 * conf/base.yaml:8-11) over one flat fp32 vector that holds every parameter field back to back,
 * in place.  group_end[k] (HOST array, ascending, last == n) closes parameter group k, group_lr[k]
 * (HOST) is its learning rate for this step; step counts from 1.  At most 8 groups. */
/* gsgen_project_gaussians_backward_batch behind the fused RGB + heads compositing (gsgen_vol_render_rgbd_backward_batch): takes
 * each view's channel gradients g_chan6[v] [N,6] = d L / d (r, g, b, depth, 1, depth^2) and its depths depth[v] [N] and forms
 * d L / d depth = g3 + 2 depth g5 itself (the depth head and the depth^2 head, gs/gaussian_splatting.py:1334-1403), and writes
 * the colour gradient g_color [N,3] = sum over the views of g_chan6[v][:, 0:3] in the same pass -- the two torch kernels the
 * caller ran between the compositing backward and the projection backward.  Rows a view's mask excludes contribute nothing. */
int gsgen_project_gaussians_backward_batch_heads(uint32_t n_views, uint32_t N, const float *mean, const float *qvec,
                                                 const float *svec, const float *const *c2w, int detach_depth,
                                                 const uint8_t *const *mask, const float *const *g_mean2d,
                                                 const float *const *g_cov2d, const float *const *g_chan6,
                                                 const float *const *depth, float *g_mean, float *g_qvec, float *g_svec,
                                                 float *g_color, gsgen_stream_t stream);
/* The same behind the MOMENT form of that compositing backward (gsgen_vol_render_rgbd_backward_batch_moments, round 6):
 * g_mom2[v] [N,2] = (Mu, Mv) and g_mom4[v] [N,4] = (Muu, Muv, Mvv, -) are sums over the view's pixels of the per-pixel weight
 * g = d L / d (a G) * a G against the whitened offsets (u, v) of the Cholesky-form Gaussian; with Sigma^-1 d = (k0 u, k1 u + k2 v),
 * k from the view's cov2d[v] [N,2,2] exactly as the compositing kernels prepare it, the reference's sums (kernels.h:394-418)
 *   d mean2d = (k0 Mu, k1 Mu + k2 Mv),  d cov2d = 0.5 [k0^2 Muu, k0 (k1 Muu + k2 Muv); same, k1^2 Muu + 2 k1 k2 Muv + k2^2 Mvv]
 * are formed here in fp64, once per (view, Gaussian), and chained through the projection as above.  g_chan6[v][:, 3] holds the
 * folded d L / d depth of the three depth heads (columns 4, 5 stay zero).  g_mom2[v] is OVERWRITTEN with the view's
 * d L / d mean2d (what gsgen_densify_update_batch reads, gs/gaussian_splatting.py:464-469). */
/* ... and behind the SH kernels' moment form (gsgen_vol_render_backward_sh_batch_routed_moments): g_mom2[v] = sum g (tx, ty),
 * g_mom4[v] = sum g (tx tx, tx ty, ty ty, -) with (tx, ty) = det Sigma^-1 d; d mean2d = M1 / det, d cov2d = 0.5 M2 / det^2 with the
 * fp32 determinant of cov2d[v] the kernels use (kernels.h:179).  g_mom2[v] is overwritten with d L / d mean2d as above. */
int gsgen_project_gaussians_backward_batch_moments_sh(uint32_t n_views, uint32_t N, const float *mean, const float *qvec,
                                                      const float *svec, const float *const *c2w, int detach_depth,
                                                      const uint8_t *const *mask, float *const *g_mom2,
                                                      const float *const *g_mom4, const float *const *cov2d, float *g_mean,
                                                      float *g_qvec, float *g_svec,
                                                      float *stat_grad_accum /* or NULL: [N], += sum over the views of |d L / d mean2d| */,
                                                      float *stat_cnt /* or NULL: [N], += the views that saw the Gaussian (gs/gaussian_splatting.py:464-469) */,
                                                      gsgen_stream_t stream);
int gsgen_project_gaussians_backward_batch_heads_moments(uint32_t n_views, uint32_t N, const float *mean, const float *qvec,
                                                         const float *svec, const float *const *c2w, int detach_depth,
                                                         const uint8_t *const *mask, float *const *g_mom2,
                                                         const float *const *g_mom4, const float *const *g_chan6,
                                                         const float *const *depth, const float *const *cov2d,
                                                         const float *const *chol /* or NULL: the views' gsgen_geometry_view::chol */,
                                                         float *g_mean, float *g_qvec, float *g_svec, float *g_color,
                                                         float *stat_grad_accum /* or NULL, as above */, float *stat_cnt /* or NULL */,
                                                         gsgen_stream_t stream);
/* The model's parameter activations (utils/activations.py:36-57; svec / alpha / color = act(raw), gs/gaussian_splatting.py:113-124) for
 * all three fields in one launch, and their backward in one (g_* hold d L / d activated on entry, d L / d raw on return).  Codes:
 * 0 nothing, 1 exp, 2 sigmoid, 3 abs, 4 relu, 5 softplus, 6 biased_relu, 7 biased_abs.  svec / color are [N,3], alpha [N].  The
 * reference runs three torch kernels forward and three autograd nodes backward per step: host time, not device time. */
int gsgen_activate_fields(uint32_t N, const float *svec_raw, const float *alpha_raw, const float *color_raw, int svec_act,
                          int alpha_act, int color_act, float *svec, float *alpha, float *color, gsgen_stream_t stream);
int gsgen_activate_fields_backward(uint32_t N, const float *svec_raw, const float *alpha_raw, const float *color_raw,
                                   const float *svec, const float *alpha, const float *color, int svec_act, int alpha_act,
                                   int color_act, float *g_svec, float *g_alpha, float *g_color, gsgen_stream_t stream);
int gsgen_adam_step(uint64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                    uint32_t n_groups, const uint64_t *group_end, const float *group_lr, float beta1,
                    float beta2, float eps, uint32_t step, gsgen_stream_t stream);
/* The same step with its per-step scalars read from DEVICE memory, so that a captured hipGraph of an optimisation step replays with
 * the learning rates and bias corrections of the step it is replayed for (gsgen_amd.graph.CapturedStep; gsgen_adam_step bakes them
 * into its kernel arguments).  scalars [9] (device): step_size of group 0 .. 7 (lr / (1 - beta1^step), unused groups ignored) and, at
 * [8], sqrt(1 - beta2^step) -- the nine floats gsgen_adam_step_scalars computes on the HOST (same double arithmetic as
 * gsgen_adam_step) into out9 for the caller to copy there. */
int gsgen_adam_step_scalars(uint32_t n_groups, const float *group_lr, float beta1, float beta2, uint32_t step, float *out9);
int gsgen_adam_step_device_scalars(uint64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                   uint32_t n_groups, const uint64_t *group_end, float beta1, float beta2, float eps,
                                   const float *scalars, gsgen_stream_t stream);
/* Densification statistics of one camera (gs/gaussian_splatting.py:1240-1245, :464-469), rows
 * aligned with mask [N] (NULL = all rows):
 *   max_radii2d[i] = max(max_radii2d[i], m + sqrt(max(m^2 - det(cov2d_i), 0))), m = tr/2
 *   grad_accum[i] += |grad_mean2d_i|_2 ;  cnt[i] += 1
 * A NaN radius (NaN trace) sticks in max_radii2d, as torch.max does, also through later calls; a negative one never raises it.
 * Either pair (cov2d, max_radii2d) / (grad_mean2d, grad_accum[, cnt]) may be NULL together.
 * torch.det's LU rounding is not reproduced: det = c00*c11 - c01*c10 in fp32. */
int gsgen_densify_update(uint32_t N, const float *cov2d, const float *grad_mean2d,
                         const uint8_t *mask, float *max_radii2d, float *grad_accum, float *cnt,
                         gsgen_stream_t stream);
/* The same for the cameras of a batch in ONE launch (maximum / sum / count folded over the views in
 * registers, then one atomic each per Gaussian).  cov2d / grad_mean2d / mask: HOST arrays of n_views DEVICE
 * pointers, read before the call returns; the NULL conventions of gsgen_densify_update apply to the arrays
 * (mask may also be NULL per view). */
int gsgen_densify_update_batch(uint32_t n_views, uint32_t N, const float *const *cov2d,
                               const float *const *grad_mean2d, const uint8_t *const *mask, float *max_radii2d,
                               float *grad_accum, float *cnt, gsgen_stream_t stream);
/* AABB tile rectangles + pair count on the device (gs/culling.py:8-37 without the .item()
 * host sync): writes aabb_topleft/bottomright int32 [N,2] and *total (device uint32, zeroed
 * inside the call) = N_with_dub. */
int gsgen_tile_culling_aabb_count(uint32_t N, const float *mean2d, const float *cov2d,
                                  uint32_t tile_size, float fx, float fy, float cx, float cy,
                                  uint32_t w, uint32_t h, float D, int *aabb_topleft,
                                  int *aabb_bottomright, uint32_t *total, gsgen_stream_t stream);

/* ---- the reference's older binning pipeline (compat: GaussianRenderer, gs/debug.py, gs/benchmarks.py) ----
 * mode 0: a Gaussian belongs to a tile when its value at one of the four tile corners exceeds thresh
 * (count_num_gaussians_each_tile / image_sort: render.cu:46-70,139-176, tile_ops.h, kernels.h:253-272;
 * cov_or_radius = cov [N,2,2]); mode 1: when its bounding circle reaches the tile
 * (count_num_gaussians_each_tile_bcircle / prepare_image_sort: render.cu:73-137, culling.h:48-130,
 * kernels.h:306-350; cov_or_radius = radius [N]).
 * count: num_gaussians[tile] += hits (int32 [T], caller-zeroed).
 * image_sort: offset[T] = exclusive scan of the incoming tile_n_gaussians; tiledepth [N_with_dub] receives
 * the {lo = float depth, hi = tile} keys in fill order (per tile, ascending Gaussian index) and is left
 * unsorted, as in the reference; gaussian_ids [N_with_dub] receives the ids sorted per tile by depth;
 * mode 0 rewrites tile_n_gaussians with its own count.  Workspace from the caller. */
int gsgen_legacy_count_tiles(uint32_t mode, uint32_t N, const float *mean, const float *cov_or_radius,
                             const float *topleft, uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w,
                             float pixel_size_x, float pixel_size_y, float thresh, int *num_gaussians,
                             gsgen_stream_t stream);
size_t gsgen_legacy_sort_workspace_bytes(uint32_t N_with_dub, uint32_t n_tiles);
int gsgen_legacy_image_sort(uint32_t mode, uint32_t N, uint32_t N_with_dub, int *gaussian_ids,
                            unsigned long long *tiledepth, const float *depth, int *tile_n_gaussians, int *offset,
                            const float *mean, const float *cov_or_radius, const float *topleft, uint32_t tile_size,
                            uint32_t n_tiles_h, uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                            float thresh, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* Fused frame: frustum cull + projection + AABB + binning + per-tile sort in one enqueue with
 * no host round trip (gs/gaussian_splatting.py:1208-1295 without the mask gathers and syncs).
 * `cam` (DEVICE, 56 floats): [0..11] c2w row-major 3x4; [12..15] fx, fy, cx, cy;
 * [16] frustum_culling_radius (<= 0: skip the cull); [17] tile_culling_radius (the reference's
 * D = 6.0); [18..19] spare; [20..37] frustum plane normals [6,3]; [38..55] plane points [6,3]
 * (both as utils/camera.py:260-294 computes them; gsgen_pack_camera fills the block on the host).
 * Culled Gaussians keep their index and emit no pairs.  gaussian_ids has capacity D_cap; the
 * true pair count is written to *total (device); if it exceeds D_cap nothing is binned,
 * start/end are all GSGEN_LIST_OVERFLOW (-2) and *total still holds the required size.  A frame that does not fit is never
 * rendered as a finite blank image: every compositing FORWARD of this library writes NaN into out (all channels) and T for a
 * tile whose start is GSGEN_LIST_OVERFLOW -- loss and image are visibly dead --, every backward skips such a tile.  (The
 * reference sizes gaussian_ids exactly after a host sync, gs/culling.py:34, and has no such state; -1 stays "empty tile",
 * aabb_culling.h:248-249.)
 * pair_report (gsgen_frame_geometry_report, gsgen_geometry_view::pair_report; optional): two uint32 in HOST-visible memory
 * (pinned + device-mapped, e.g. hipHostMalloc) that the geometry launch writes with system-scope stores: [0] = this frame's
 * pair count (every frame: a caller can grow the list BEFORE it overflows), [1] = max(count) over the frames that did not
 * fit (kept until the host clears it).  No copy, no event, no sync; a hipGraph replay reports the same way. */
#define GSGEN_LIST_OVERFLOW (-2)
size_t gsgen_frame_workspace_bytes(uint32_t N, uint32_t D_cap, uint32_t n_tiles);
/* Small host -> device upload THROUGH KERNEL ARGUMENTS (per-render constants: camera blocks, pixel origins): the bytes
 * travel in the dispatch packets of one-workgroup kernels (3 584 bytes each), so the host buffer may be reused as soon
 * as the call returns, nothing is staged or pinned, the call does not wait for the stream and can be captured into a
 * hipGraph.  dst (device) and bytes must be multiples of 4.  No counterpart in the reference (it uploads with
 * torch's `.to(device)` per camera). */
int gsgen_upload_small(void *dst, const void *host_src, size_t bytes, gsgen_stream_t stream);
/* HOST helper: the 68-float per-camera blocks this library's fused paths upload (gsgen_upload_small) for n cameras in
 * one call: cam[56] as gsgen_pack_camera | pixel origin (-cx/fx, -cy/fy) | the 9 rotation entries of c2w, row-major |
 * pad.  c2w: n poses of >= 12 floats (rows of [R|t]), c2w_stride floats apart; intr: [n,8] doubles fx fy cx cy w h near
 * far. */
int gsgen_pack_camera_blocks(uint32_t n, const float *c2w, uint32_t c2w_stride, const double *intr,
                             float frustum_radius, float tile_radius, float *blocks);
/* HOST helper (no device work): fills cam[56] from a host c2w [3,4] and the CameraInfo fields
 * (utils/camera.py:219-259; yfov = 2 atan(h / 2fy), aspect = w / h). */
int gsgen_pack_camera(const float *c2w, float fx, float fy, float cx, float cy, uint32_t w, uint32_t h,
                      double near_plane, double far_plane, float frustum_radius, float tile_radius,
                      float *cam);
int gsgen_frame_geometry(uint32_t N, const float *mean, const float *qvec, const float *svec,
                         const float *cam, uint32_t W, uint32_t H, uint32_t D_cap, float *mean2d,
                         float *cov2d, float *depth, uint8_t *mask, int *gaussian_ids, int *start,
                         int *end, uint32_t *total, void *workspace, size_t workspace_bytes,
                         gsgen_stream_t stream);
/* HOST helper: the device-side address of a pinned (hipHostMalloc / torch pin_memory) host block, for pair_report; NULL when the
 * block is not mapped into the device's address space. */
void *gsgen_host_device_pointer(void *pinned_host);
int gsgen_frame_geometry_report(uint32_t N, const float *mean, const float *qvec, const float *svec,
                                const float *cam, uint32_t W, uint32_t H, uint32_t D_cap, float *mean2d,
                                float *cov2d, float *depth, uint8_t *mask, int *gaussian_ids, int *start,
                                int *end, uint32_t *total, uint32_t *pair_report, void *workspace,
                                size_t workspace_bytes, gsgen_stream_t stream);

/* gsgen_frame_geometry for the B cameras of a batch in ONE enqueue of the same eight kernels
 * (gridDim.y / .z = view) instead of eight small launches per camera: a single view's launches are
 * latency-bound (100k Gaussians, 2.5k tiles do not fill 256 CUs; 108 us end to end on cfg2, ~45 us per
 * view however many streams overlap them), B views per launch fill the chip.  Per view the outputs are
 * bit-identical to gsgen_frame_geometry.  `views` is HOST memory, read before the call returns; each
 * view brings its own outputs, pair capacity and gsgen_frame_workspace_bytes(N, D_cap, n_tiles)
 * workspace (gsgen_frame_tile_order applies to it unchanged).  batch_workspace: device,
 * gsgen_frame_batch_workspace_bytes(n_views) bytes, not reused before the enqueued work has run. */
typedef struct gsgen_geometry_view {
  const float *cam;                        /* DEVICE, 56 floats as for gsgen_frame_geometry */
  float *mean2d, *cov2d, *depth;           /* [N,2], [N,2,2], [N] */
  uint8_t *mask;                           /* [N] */
  int *gaussian_ids, *start, *end;         /* [D_cap], [n_tiles], [n_tiles] */
  uint32_t *total;                         /* [1] */
  void *workspace;
  size_t workspace_bytes;
  uint32_t D_cap;
  /* optional (NULL = leave alone): this view's gradient accumulators of the step's backward -- d L / d mean2d [N,2] (8-byte
   * aligned), d L / d cov2d [N,2,2] (16-byte aligned), d L / d (r, g, b, depth, 1, depth^2) [N,6] (8-byte aligned) -- ZERO-FILLED
   * by the projection launch, which writes a record per Gaussian of the view anyway: the compositing backward kernels
   * accumulate into caller-zeroed arrays (as the reference's, vol_render.h:866-992), and the fill between forward and
   * backward was a launch of its own in every step's chain */
  float *zero_grad_mean2d, *zero_grad_cov2d, *zero_grad_chan6;
  uint32_t *pair_report;                   /* optional, HOST-visible [2]: see "pair_report" above */
  /* optional (round 6): [N,4] floats, 16-byte aligned -- the projection launch also prepares the evaluation record of the RGB / scalar /
   * RGB + heads compositing kernels once per Gaussian of the view: (p0, p1, p2) = sqrt(0.5 log2 e) * the Cholesky factor of the
   * symmetrised Sigma^-1, formed in fp64 from cov2d and rounded to fp32, and a validity flag (0 for a degenerate or non-finite
   * covariance).  gsgen_rgbd_view::chol hands it to the compositing launches. */
  float *chol;
  /* optional (round 6): [N] floats shared by the views of every batch -- the projection launch raises them to each visible Gaussian's
   * screen-space radius m + sqrt(max(m^2 - det, 0)), m = (c0 + c3) / 2 of this view's cov2d: the `max_radii2d` statistic the trainer's prune
   * step reads (gs/gaussian_splatting.py:1240-1245), what gsgen_densify_update_batch(cov2d, ...) computes in a launch of its own */
  float *max_radii2d;
} gsgen_geometry_view;
size_t gsgen_frame_batch_workspace_bytes(uint32_t n_views);
int gsgen_frame_geometry_batch(uint32_t n_views, const gsgen_geometry_view *views, uint32_t N, const float *mean,
                               const float *qvec, const float *svec, uint32_t W, uint32_t H,
                               void *batch_workspace, gsgen_stream_t stream);
/* The same, and the launch also zero-fills `zero_shared` (zero_shared_floats floats: a multiple of 4, 16-byte aligned; 0 = none):
 * the gradient accumulators the views of the batch SHARE (d L / d alpha [N] and d L / d sh [N,3,C*C] or d L / d colour, laid out
 * back to back by the caller).  With the per-view targets above no fill kernel is left between a step's forward and backward. */
int gsgen_frame_geometry_batch_zero(uint32_t n_views, const gsgen_geometry_view *views, uint32_t N, const float *mean,
                                    const float *qvec, const float *svec, uint32_t W, uint32_t H, float *zero_shared,
                                    size_t zero_shared_floats, void *batch_workspace, gsgen_stream_t stream);

/* Launch order for the compositing kernels produced by gsgen_frame_geometry: a device array
 * of n_tiles tile indices, longest list first (pointer into `workspace`; pure host arithmetic).
 * The *_ordered variants of the SH compositing entry points take it (NULL = spatial order);
 * they are otherwise identical to gsgen_vol_render_sh / gsgen_vol_render_backward_sh. */
const uint32_t *gsgen_frame_tile_order(void *workspace, uint32_t N, uint32_t D_cap, uint32_t n_tiles);
/* How many (Gaussian, tile) keys of one 2 048-Gaussian chunk the batched binning groups by tile in LDS before it stores them
 * (gsgen_amd/csrc/binning.hip, bin_push_body): a chunk with more keeps its leading tiles' keys there and stores the others one
 * by one.  A constant of the build (images of more than 4 080 tiles stage less: the workgroup's LDS stays within 64 KB);
 * the lists do not depend on it.  For tests that place a chunk on either side of it. */
uint32_t gsgen_emit_stage_capacity(void);
int gsgen_vol_render_sh_ordered(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                const float *sh_coeffs, const float *alpha, const int *start,
                                const int *end, const int *gaussian_ids, float *out, const float *topleft,
                                const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                                uint32_t W, uint32_t C, float thresh, const float *bg_rgb, float *T,
                                const uint32_t *tile_order, gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_ordered(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                         const float *sh_coeffs, const float *alpha, const int *start,
                                         const int *end, const int *gaussian_ids, const float *out,
                                         float *grad_mean, float *grad_cov, float *grad_sh_coeffs,
                                         float *grad_alpha, const float *grad_out, const float *topleft,
                                         const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                         uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                         uint32_t H, uint32_t W, uint32_t C, float thresh,
                                         const float *bg_rgb, const uint32_t *tile_order,
                                         gsgen_stream_t stream);

/* Segmented backward.  The compositing backward normally runs one workgroup per tile, and the
 * launch ends on the few heaviest tiles.  Given a segment workspace, the FORWARD additionally
 * stores the per-pixel state (transmittance, prefix colour) in front of every 32nd list entry and
 * the entry at which each pixel saturated; the BACKWARD then runs one workgroup per (tile,
 * 32-entry segment) -- uniform work units, n_segments per tile (the last one takes whatever
 * remains).  Same results up to the rounding of `final - prefix`.  n_segments <= 1 or a NULL
 * workspace: exactly the *_ordered entry points.  The workspace written by the forward must be
 * handed unchanged to the backward of the same frame. */
size_t gsgen_segment_workspace_bytes(uint32_t n_tiles, uint32_t n_segments);
int gsgen_vol_render_sh_segmented(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                  const float *sh_coeffs, const float *alpha, const int *start,
                                  const int *end, const int *gaussian_ids, float *out, const float *topleft,
                                  const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                  uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                                  uint32_t W, uint32_t C, float thresh, const float *bg_rgb, float *T,
                                  const uint32_t *tile_order, void *segment_workspace, uint32_t n_segments,
                                  gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_segmented(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                           const float *sh_coeffs, const float *alpha, const int *start,
                                           const int *end, const int *gaussian_ids, const float *out,
                                           float *grad_mean, float *grad_cov, float *grad_sh_coeffs,
                                           float *grad_alpha, const float *grad_out, const float *topleft,
                                           const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                           uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                           uint32_t H, uint32_t W, uint32_t C, float thresh,
                                           const float *bg_rgb, const uint32_t *tile_order,
                                           const void *segment_workspace, uint32_t n_segments,
                                           gsgen_stream_t stream);

/* Batched cameras in ONE launch (the reference loops over the cameras of a batch in
 * Python, gs/gaussian_splatting.py:1423-1466, calling render_sh / its backward once per camera).  A
 * single 800x800 launch ends on a tail of long sparse tiles that leaves most of the chip idle;
 * one launch per (at most 8) views pays that tail once per batch.  Every view has its own projected records,
 * lists and outputs; sh_coeffs / alpha and their gradients are shared, the gradients accumulating
 * atomically over views exactly as they do over tiles.  Per view the result is bit-identical to
 * gsgen_vol_render_sh_segmented / gsgen_vol_render_backward_sh_segmented on the same inputs
 * (gradient sums up to fp32 atomic order).  `views` is HOST memory, read before the call returns.
 * batch_workspace: device, gsgen_sh_batch_workspace_bytes(n_views) bytes, one per batch in flight.  (Since round 4 the per-view
 * kernel parameters travel in the kernel arguments, 8 views per launch, and the plain batched entry points no longer write
 * to it; the routed ones keep their per-tile routing bytes behind it -- size and argument stay for ABI stability.)
 * The batched forward writes EVERY pixel of out / T: empty tiles receive bg_rgb (0 without one) and T = 1, so the caller
 * need not pre-initialise the images (the per-camera entry points keep the reference's contract, vol_render.h:1006-1013). */
typedef struct gsgen_sh_view {
  const float *mean, *cov;                 /* [N,2], [N,2,2] of this view */
  const int *start, *end, *gaussian_ids;   /* [n_tiles], [n_tiles], [D] */
  const uint32_t *tile_order;              /* [n_tiles] or NULL (then NULL in every view) */
  const float *topleft, *c2w;              /* [2], [9] */
  const float *bg_rgb;                     /* [3] or NULL */
  float pixel_size_x, pixel_size_y;
  float *out, *T;                          /* [H,W,3], [H,W]; out is read by the backward */
  void *segment_workspace;                 /* gsgen_segment_workspace_bytes, or NULL if n_segments <= 1 */
  const float *grad_out;                   /* backward: [H,W,3] */
  float *grad_mean, *grad_cov;             /* backward: [N,2], [N,2,2] of this view, accumulated into */
  /* Round 6, optional (zero = as before), the *_routed launches with per-splat bounds (sh_row_bounds) only -- the persistent exact
   * fallback kernels are launched only when they may have something to do:
   *   route_report: one uint32 in HOST-visible memory (pinned + device-mapped, as pair_report): the polynomial forward stores 1 there
   *     whenever a tile's staged batch holds more than a quarter of splats beyond the bound -- the condition that hands the tile to the
   *     exact fallback.  No copy, no event, no sync; the host reads (and clears) it before a later batch.
   *   no_fallback = 1 (the same in every view, forward and backward of a batch alike): the two fallback launches are NOT enqueued and
   *     the polynomial kernels never hand a tile over -- every splat beyond the bound takes the per-entry exact tier instead, however
   *     many a tile holds.  Always correct (the same colours within the routing's 1e-5), slower on tiles crowded with such splats:
   *     meant for callers whose earlier batches reported none (gsgen_amd.BatchRenderer, bench.py: three clean reports in a row). */
  uint32_t *route_report;
  uint32_t no_fallback;
  /* optional (zero = as before; every batched SH entry point, forward and backward): DEVICE address of {pixel_size_x, pixel_size_y} of
   * this view, with the meaning of gsgen_rgbd_view::pixel_size_dev.  When set the kernels take the two from there -- once per
   * workgroup, in front of their routing decisions -- and ignore the floats above: nothing that changes from step to step then travels
   * in kernel arguments, so a captured hipGraph of an SH step can be replayed for other cameras (poses AND intrinsics: the reference
   * samples a focal length per step, data/__init__.py:194) once their camera blocks and these floats are in place
   * (gsgen_amd.graph.CapturedStep).  Set in every view of a launch or in none (GSGEN_EINVAL otherwise, nothing is enqueued): such a
   * launch runs its own instantiations of the kernels, and the host-side shortcut of the bounded entry points ("no view of this batch
   * can be polynomial: launch the exact kernels alone") is skipped -- the host does not know the floats; every workgroup decides. */
  const float *pixel_size_dev;
} gsgen_sh_view;
size_t gsgen_sh_batch_workspace_bytes(uint32_t n_views);
int gsgen_vol_render_sh_batch(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                              const float *sh_coeffs, const float *alpha, uint32_t tile_size,
                              uint32_t n_tiles_h, uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C,
                              float thresh, uint32_t n_segments, void *batch_workspace,
                              gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_batch(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                       const float *sh_coeffs, const float *alpha, float *grad_sh_coeffs,
                                       float *grad_alpha, uint32_t tile_size, uint32_t n_tiles_h,
                                       uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C, float thresh,
                                       uint32_t n_segments, void *batch_workspace, gsgen_stream_t stream);

/* ---- the coefficient bound: the fast form of the per-pixel SH basis, decided ON THE DEVICE ----------------------------
 * The reference evaluates the SH basis per pixel for dir = normalize(R (qx, qy, 1)) (vol_render_sh.h:48-65).  Inside a
 * 16 x 16 tile that is a degree-2 polynomial in the pixel offsets to within 1.0 delta^3 of a basis value (delta = the tile's
 * half diagonal in camera space; the fit that ships reaches 0.93 delta^3 -- tests/test_poly_fit_bound.py sweeps it over rotations,
 * tile positions and focal lengths): six-term contractions against coefficients transformed once per (tile, splat), +56 %
 * renders/s on BASELINE configs[1].  The colour error is <= 0.25 * S * delta^3 with
 *     S = max over splats and channels of sum_{k >= 1} |sh[i][c][k]|,
 * and the polynomial form is used only where that stays <= 1e-5 - 8.7e-7.  The 8.7e-7 belong to the Taylor tier (round 5): a
 * splat whose logits move little enough across the tile -- remainder bound 0.00694 (l + q)^3 + 0.02312 q (2 l + q) <= 8.7e-7
 * for the linear and quadratic parts l, q of its row's coefficient sum, the ordinary case by a factor of hundreds -- gets its
 * COLOUR as a quadratic in the pixel offsets, formed once per (tile, splat): no exponential per pixel.  Together: routed colours
 * within 1e-5 of the exact kernels', a tenth of the 1e-4 image tolerance.  (Rounds 2-4 routed on 0.7 delta^3, a calibration
 * of a different interpolation: 1.4e-5.)
 *
 * S lives in DEVICE memory and never visits the host: gsgen_sh_l1_bound writes it (one coalesced pass over the
 * coefficients, ~5 us for 100 k splats; enqueue it on the render's stream whenever the coefficients may have changed, i.e.
 * every optimiser step), the *_bounded entry points below take its device address.  With a bound (SH degree 3 only) they
 * enqueue the polynomial-basis kernel AND the exact one over the same grid; every workgroup reads S and its view's pixel
 * size and exactly one of the two kernels renders the view -- no host decision, no synchronisation, hipGraph-capturable, and
 * a bound that is too large only costs speed, never accuracy.  A forward and its backward must see the same value (pass the
 * same address and do not rewrite it in between).  sh_l1_bound == NULL: the exact kernels only (gsgen_vol_render_sh_batch,
 * gsgen_vol_render_sh_segmented, ... are exactly that). */
int gsgen_sh_l1_bound(uint32_t N, const float *sh_coeffs, uint32_t C, float *out /* device, 1 float, OVERWRITTEN */,
                      gsgen_stream_t stream);
/* Debug verification of a bound some other pass produced (e.g. a fused optimiser step): *n_violations (device uint32,
 * OVERWRITTEN) = the number of (splat, channel) rows whose sum_{k >= 1} |sh| exceeds *bound (device). */
int gsgen_sh_l1_bound_check(uint32_t N, const float *sh_coeffs, uint32_t C, const float *bound, uint32_t *n_violations,
                            gsgen_stream_t stream);
/* HOST arithmetic only: 1 if a view of this pixel size (max of pixel_size_x / _y) takes the polynomial form under the
 * bound value S -- the device's own rule, for reports */
int gsgen_sh_poly_applies(float sh_l1_bound, float max_pixel_size, uint32_t C);
int gsgen_vol_render_sh_batch_bounded(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                      const float *sh_coeffs, const float *alpha, uint32_t tile_size,
                                      uint32_t n_tiles_h, uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C,
                                      float thresh, uint32_t n_segments, const float *sh_l1_bound /* device or NULL */,
                                      void *batch_workspace, gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_batch_bounded(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                               const float *sh_coeffs, const float *alpha, float *grad_sh_coeffs,
                                               float *grad_alpha, uint32_t tile_size, uint32_t n_tiles_h,
                                               uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C, float thresh,
                                               uint32_t n_segments, const float *sh_l1_bound /* device or NULL */,
                                               void *batch_workspace, gsgen_stream_t stream);
/* One camera (gsgen_vol_render_sh_segmented / gsgen_vol_render_backward_sh_segmented + the bound): what the `_gs` SH names
 * (tile_based_vol_rendering_sh / _backward_sh and their _with_bg forms, gs/src/render.h:83-127) run on -- the binding
 * computes S into a scratch float in front of each call, so the reference's call shape gets the fast kernels too. */
int gsgen_vol_render_sh_bounded(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                const float *sh_coeffs, const float *alpha, const int *start,
                                const int *end, const int *gaussian_ids, float *out, const float *topleft,
                                const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                                uint32_t W, uint32_t C, float thresh, const float *bg_rgb, float *T,
                                const uint32_t *tile_order, void *segment_workspace, uint32_t n_segments,
                                const float *sh_l1_bound /* device or NULL */, gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_bounded(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                         const float *sh_coeffs, const float *alpha, const int *start,
                                         const int *end, const int *gaussian_ids, const float *out,
                                         float *grad_mean, float *grad_cov, float *grad_sh_coeffs,
                                         float *grad_alpha, const float *grad_out, const float *topleft,
                                         const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                         uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                         uint32_t H, uint32_t W, uint32_t C, float thresh,
                                         const float *bg_rgb, const uint32_t *tile_order,
                                         const void *segment_workspace, uint32_t n_segments,
                                         const float *sh_l1_bound /* device or NULL */, gsgen_stream_t stream);

/* ---- per-TILE routing of the polynomial SH basis (round 4) ------------------------------------------------------------------
 * The *_bounded entry points above route per VIEW on one number, the scene's largest per-row coefficient sum: one splat with large
 * higher-band coefficients, or a wide camera, sends the whole view to the exact kernels.  The *_routed entry points take the
 * bound per SPLAT -- sh_row_bounds[i] = max over the three channels of sum_{k >= 1} |sh[i][c][k]|, DEVICE memory, [N], measured per
 * step by gsgen_sh_l1_bound_rows (one coalesced pass, no atomics but one per workgroup; out_max, optional, receives the global
 * maximum the per-view rule uses) -- and decide per ENTRY and per TILE: a splat that satisfies 0.25 * S_i * delta^3 <= 1e-5 - 8.7e-7
 * for its view's pixel size (the same rule, per splat) is evaluated through the tile's polynomial form; one beyond it is evaluated
 * exactly, entry by entry, inside the same kernel (the pixel's own SH basis against its raw coefficients); a staged batch of 32
 * records with more than a quarter of such splats sends its tile -- and only that tile -- to the exact kernel.  Splats behind the
 * point where the tile's pixels saturate are never staged and never count.  Batched launches record the decision in one byte per (view, tile)
 * inside batch_workspace (gsgen_sh_batch_workspace_bytes_routed): the polynomial forward writes it, the exact fallback behind it
 * and both backward kernels read it, so forward and backward agree by construction; per-camera launches decide before they touch
 * a tile, forward and backward alike: with sh_l1_bound given as well (the maximum gsgen_sh_l1_bound_rows leaves in out_max) a
 * view wholly within its bound -- the normal case -- takes the polynomial form without a look at the lists, otherwise the
 * tile's list is scanned against the per-splat bounds (any splat beyond them: the exact form for that tile).  sh_row_bounds == NULL: exactly the *_bounded behaviour on sh_l1_bound.  SH degree 3 only
 * (C != 4: the exact kernels).  No counterpart in the reference (vol_render_sh.h:48-65 evaluates the basis per pixel).
 *
 * The walk summary.  Behind the flag bytes (padded to 16) gsgen_sh_batch_workspace_bytes_routed reserves 17 uint32 per (view, tile):
 * `walked`, the number of list entries the polynomial forward's entry loop reached before no pixel of the tile was alive (the list's
 * length if the tile never saturated); contributed[8], bit g of word b set when entry 32 b + g reached some pixel; guarded[8], the same
 * for a trip of the threshold guard.  Bits of entries never reached are 0, and the forward writes every word of every tile it renders:
 * the workspace may arrive holding anything.  A batched launch with per-splat bounds (sh_row_bounds), SH degree 3 and n_segments <= 1
 * keeps it: gsgen_vol_render_sh_batch_routed writes the records of its views, and the polynomial kernel of
 * gsgen_vol_render_backward_sh_batch_routed / _moments runs each tile's loop to `walked`, passes the entries nobody sees and takes the
 * guard's trips from the bits instead of deciding again (entries behind the 256 of the bit words are decided there as before).  The
 * summary a backward reads is the forward's, of the same views with the same inputs, in the same workspace; any number of backward
 * launches may follow that forward.  Every other launch -- segmented, per-view bounds only, the exact kernels and their fallbacks, the
 * per-camera entry points -- neither writes nor reads it.  Size the workspace with the function: the summary is part of it. */
int gsgen_sh_l1_bound_rows(uint32_t N, const float *sh_coeffs, uint32_t C, float *out_max /* device, 1 float, or NULL */,
                           float *out_rows /* device, [N] */, gsgen_stream_t stream);
/* The same without the 4-byte fill in front of the pass (one launch less per step): running_max is only ever RAISED -- an upper
 * bound of the current coefficients' maximum as long as the caller zeroed it at some point, tight again whenever the caller
 * zeroes it (the per-view shortcut it feeds is conservative under a stale larger value, never wrong). */
int gsgen_sh_l1_bound_rows_running(uint32_t N, const float *sh_coeffs, uint32_t C, float *running_max /* device, 1 float, or NULL */,
                                   float *out_rows /* device, [N] */, gsgen_stream_t stream);
size_t gsgen_sh_batch_workspace_bytes_routed(uint32_t n_views, uint32_t n_tiles);
int gsgen_vol_render_sh_batch_routed(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                     const float *sh_coeffs, const float *alpha, uint32_t tile_size,
                                     uint32_t n_tiles_h, uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C,
                                     float thresh, uint32_t n_segments, const float *sh_l1_bound /* device or NULL */,
                                     const float *sh_row_bounds /* device [N] or NULL */, void *batch_workspace,
                                     gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_batch_routed(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                              const float *sh_coeffs, const float *alpha, float *grad_sh_coeffs,
                                              float *grad_alpha, uint32_t tile_size, uint32_t n_tiles_h,
                                              uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C, float thresh,
                                              uint32_t n_segments, const float *sh_l1_bound, const float *sh_row_bounds,
                                              void *batch_workspace, gsgen_stream_t stream);
/* The MOMENT form of gsgen_vol_render_backward_sh_batch_routed (round 6; vol_render_sh.h:353-455 / vol_render_bg.h:131-242 for the
 * cameras of a batch): same arguments and routing; the views' grad_mean [N,2] receive sum g (tx, ty), grad_cov [N,4] sum g
 * (tx tx, tx ty, ty ty; the fourth float is not written), g = d L / d (a G) * a G per pixel, (tx, ty) = det Sigma^-1 d as the
 * Gaussian is evaluated (kernels.h:172-193) -- seven packed operations per pixel pair instead of thirteen and one atomic per
 * (tile, Gaussian) less.  gsgen_project_gaussians_backward_batch_moments_sh expands them per (view, Gaussian). */
int gsgen_vol_render_backward_sh_batch_routed_moments(uint32_t n_views, const gsgen_sh_view *views, uint32_t N,
                                                      const float *sh_coeffs, const float *alpha, float *grad_sh_coeffs,
                                                      float *grad_alpha, uint32_t tile_size, uint32_t n_tiles_h,
                                                      uint32_t n_tiles_w, uint32_t H, uint32_t W, uint32_t C, float thresh,
                                                      uint32_t n_segments, const float *sh_l1_bound, const float *sh_row_bounds,
                                                      void *batch_workspace, gsgen_stream_t stream);
int gsgen_vol_render_sh_routed(uint32_t N, uint32_t D, const float *mean, const float *cov,
                               const float *sh_coeffs, const float *alpha, const int *start,
                               const int *end, const int *gaussian_ids, float *out, const float *topleft,
                               const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                               uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                               uint32_t W, uint32_t C, float thresh, const float *bg_rgb, float *T,
                               const uint32_t *tile_order, void *segment_workspace, uint32_t n_segments,
                               const float *sh_l1_bound, const float *sh_row_bounds, gsgen_stream_t stream);
int gsgen_vol_render_backward_sh_routed(uint32_t N, uint32_t D, const float *mean, const float *cov,
                                        const float *sh_coeffs, const float *alpha, const int *start,
                                        const int *end, const int *gaussian_ids, const float *out,
                                        float *grad_mean, float *grad_cov, float *grad_sh_coeffs,
                                        float *grad_alpha, const float *grad_out, const float *topleft,
                                        const float *c2w, uint32_t tile_size, uint32_t n_tiles_h,
                                        uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                                        uint32_t H, uint32_t W, uint32_t C, float thresh,
                                        const float *bg_rgb, const uint32_t *tile_order,
                                        const void *segment_workspace, uint32_t n_segments,
                                        const float *sh_l1_bound, const float *sh_row_bounds, gsgen_stream_t stream);

/* Fused RGB + auxiliary heads: what render_one does in four compositing passes
 * (gs/gaussian_splatting.py:1304-1403: rgb, depth, opacity = scalar 1, depth^2) in one.
 * out6 / grad_out6 are [H,W,6] = (r, g, b, depth, opacity, depth^2); grad_chan6 [N,6] receives the
 * gradients of the per-Gaussian channel values (r, g, b, d, 1, d*d) -- the caller folds columns
 * 3 and 5 into d/d depth (g3 + 2 d g5).  Semantics per channel are those of the single-head
 * entry points above; T as in gsgen_vol_render_start_end_with_T. */
int gsgen_vol_render_rgbd(uint32_t N, uint32_t D, const float *mean, const float *cov, const float *color,
                          const float *depth, const float *alpha, const int *start, const int *end,
                          const int *gaussian_ids, float *out6, const float *topleft, uint32_t tile_size,
                          uint32_t n_tiles_h, uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y,
                          uint32_t H, uint32_t W, float thresh, float *T, const uint32_t *tile_order,
                          gsgen_stream_t stream);
int gsgen_vol_render_rgbd_backward(uint32_t N, uint32_t D, const float *mean, const float *cov, const float *color,
                                   const float *depth, const float *alpha, const int *start, const int *end,
                                   const int *gaussian_ids, const float *out6, float *grad_mean, float *grad_cov,
                                   float *grad_chan6, float *grad_alpha, const float *grad_out6,
                                   const float *topleft, uint32_t tile_size, uint32_t n_tiles_h,
                                   uint32_t n_tiles_w, float pixel_size_x, float pixel_size_y, uint32_t H,
                                   uint32_t W, float thresh, const uint32_t *tile_order, gsgen_stream_t stream);

/* The same for the B cameras of a batch in ONE launch each way (as gsgen_vol_render_sh_batch): per-view
 * records, depths, lists, out6 / T and per-view gradients (grad_chan6 holds the view's own depth-head
 * gradients, so it is not shared); color / alpha are shared and grad_alpha accumulates over the views.
 * batch_workspace: gsgen_sh_batch_workspace_bytes(n_views), one per batch in flight. */
typedef struct gsgen_rgbd_view {
  const float *mean, *cov, *depth;         /* [N,2], [N,2,2], [N] of this view */
  const int *start, *end, *gaussian_ids;
  const uint32_t *tile_order;              /* or NULL (then NULL in every view) */
  const float *topleft;                    /* [2] */
  float pixel_size_x, pixel_size_y;
  float *out6, *T;                         /* [H,W,6], [H,W]; out6 is read by the backward */
  const float *grad_out6;                  /* backward: [H,W,6]; or NULL (heads only): the four images below */
  float *grad_mean, *grad_cov, *grad_chan6; /* backward: [N,2], [N,2,2], [N,6] of this view, accumulated into */
  /* backward of the heads with grad_out6 == NULL: d L / d rgb [H,W,3], / d depth, / d opacity, / d depth^2 [H,W] as an
   * autograd engine delivers them (one tensor per output; any may be NULL = zero) -- no [H,W,6] image to assemble */
  const float *grad_rgb, *grad_depth, *grad_opacity, *grad_depth2;
  /* Round 6, optional (zero-initialised = the layout above), RGB + heads launches only -- what the reference's model computes in
   * torch around its four compositing passes, folded into the two launches:
   *   out_rgb [H,W,3], out_depth, out_opacity, out_depth2 [H,W]: the four heads as separate contiguous images instead of out6 (all
   *     four or none; out6 may then be NULL).  The backward reads them as the forward's final image; grad_out6 must be NULL (the
   *     four-image gradient form).
   *   bg_rgb [3] (device): the forward writes rgb + T * bg (gs/renderer.py:1182; empty tiles show bg); the backward takes that sum
   *     as the final image, as the reference's does.
   *   grad_bg [64][4] (device, zeroed by the caller), backward: row (tile % 64) accumulates the tile's sum over pixels of
   *     nan_to_num(grad_rgb * T) (gs/renderer.py:1283: d L / d bg), T the forward's; the caller adds the 64 rows.
   *   depth_variance = 1: the sixth head is z_var = depth2 - depth^2 (gs/gaussian_splatting.py:1397) -- written so by the forward,
   *     and grad_depth2 is d L / d z_var (the backward forms d depth2 = g and d depth -= 2 depth g itself). */
  float *out_rgb, *out_depth, *out_opacity, *out_depth2;
  const float *bg_rgb;
  float *grad_bg;
  uint32_t depth_variance;
  /* optional (rgbd and rgb launches): the view's prepared evaluation records [N,4] as gsgen_geometry_view::chol delivers them -- staging
   * then reads 16 bytes per record instead of running the fp64 Cholesky preparation (kernels.h:195-224 evaluates the quadratic form in
   * fp64; here its factor is prepared in fp64) per staged (tile, Gaussian) record in the forward and again in the backward */
  const float *chol;
  /* optional (batched launches): DEVICE address of {pixel_size_x, pixel_size_y} of this view.  When set the kernels take the two from
   * there and ignore the floats above: nothing that changes from step to step then travels in kernel arguments, so a captured
   * hipGraph of the step can be replayed for other cameras (poses AND intrinsics: the reference samples a focal length per step,
   * data/__init__.py:194) once their camera blocks and these floats are in place (gsgen_amd.graph.CapturedStep). */
  const float *pixel_size_dev;
} gsgen_rgbd_view;
/* The batched forwards (rgbd and rgb) write EVERY pixel of out6 / T, empty tiles included (channels 0, T = 1): the caller need
 * not pre-initialise the images (the per-camera entry points above keep the reference's contract: empty tiles are left alone). */
int gsgen_vol_render_rgbd_batch(uint32_t n_views, const gsgen_rgbd_view *views, uint32_t N, const float *color,
                                const float *alpha, uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w,
                                uint32_t H, uint32_t W, float thresh, void *batch_workspace,
                                gsgen_stream_t stream);
int gsgen_vol_render_rgbd_backward_batch(uint32_t n_views, const gsgen_rgbd_view *views, uint32_t N,
                                         const float *color, const float *alpha, float *grad_alpha,
                                         uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w, uint32_t H,
                                         uint32_t W, float thresh, void *batch_workspace, gsgen_stream_t stream);
/* The MOMENT form of gsgen_vol_render_rgbd_backward_batch (round 6; replaces vol_render.h:866-992 + vol_render_scalar.h:104-234
 * for the trainer's default outputs, gs/gaussian_splatting.py:1304-1416).  Same arguments; what the per-view accumulators
 * receive differs: grad_mean [N,2] the two first moments (Mu, Mv), grad_cov [N,4] the three second moments (Muu, Muv, Mvv; the
 * fourth float is not written) of the per-pixel weight d L / d (a G) * a G against the whitened offsets u = p0 x + p1 y,
 * v = p2 y of the Cholesky-form Gaussian, grad_chan6 [N,6] = (d r, d g, d b, d L / d depth with the depth^2 head folded in
 * -- sum w (go_d + 2 d go_dd) --, untouched, untouched).  gsgen_project_gaussians_backward_batch_heads_moments expands them: the
 * entry loop sums 10 components per (tile, Gaussian) instead of 13 and spends 14 packed operations on the geometric part
 * instead of 29.  Gradients agree with the plain form to fp32 rounding (tests/test_cpu_host.py, tests/test_gpu_api.py). */
int gsgen_vol_render_rgbd_backward_batch_moments(uint32_t n_views, const gsgen_rgbd_view *views, uint32_t N,
                                                 const float *color, const float *alpha, float *grad_alpha,
                                                 uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w, uint32_t H,
                                                 uint32_t W, float thresh, void *batch_workspace, gsgen_stream_t stream);
/* Post-activation RGB only (gsgen_vol_render_start_end_with_T / gsgen_vol_render_backward_start_end for the
 * cameras of a batch): the same view array with out6 / grad_out6 read as [H,W,3] images, depth and grad_chan6
 * unused (may be NULL); the colour gradient [N,3] is shared and accumulates over the views like grad_alpha. */
int gsgen_vol_render_rgb_batch(uint32_t n_views, const gsgen_rgbd_view *views, uint32_t N, const float *color,
                               const float *alpha, uint32_t tile_size, uint32_t n_tiles_h, uint32_t n_tiles_w,
                               uint32_t H, uint32_t W, float thresh, void *batch_workspace, gsgen_stream_t stream);
int gsgen_vol_render_rgb_backward_batch(uint32_t n_views, const gsgen_rgbd_view *views, uint32_t N,
                                        const float *color, const float *alpha, float *grad_color,
                                        float *grad_alpha, uint32_t tile_size, uint32_t n_tiles_h,
                                        uint32_t n_tiles_w, uint32_t H, uint32_t W, float thresh,
                                        void *batch_workspace, gsgen_stream_t stream);

/* ---- exact k-nearest neighbours (gsgen_amd/csrc/knn.hip) --------------------------------------------------------
 * replaces pytorch3d's knn_points as utils/ops.py:104-134 calls it (and faiss IndexFlatL2, utils/initialize.py:16-35).
 * points [n_points,3] fp32; every point is also a query.  Row i of dist2 [n_points,K] fp32 / idx [n_points,K] int32 lists the K
 * nearest points in ascending (dist2, index) order, dist2 = dx*dx + dy*dy + dz*dz with d = p_j - p_i evaluated left to right
 * (an fp32 brute force reproduces every bit); row i holds i itself at distance 0, after any lower-index exact duplicate.
 * A point with a NaN / Inf coordinate is nobody's neighbour; its own row, and every row with fewer than K finite candidates, is
 * padded with idx -1, dist2 +inf.  K in 1..32 (else GSGEN_EUNSUPPORTED); n_points == 0 or K > n_points: GSGEN_EINVAL.
 * workspace: device, gsgen_knn_workspace_bytes(n_points, K) bytes (0 for an unsupported pair).  Grid bounds and counts are
 * computed on the device and the launch shapes depend on (n_points, K) alone: no host synchronisation, so the call can be
 * captured in a hipGraph and replayed on new values of the same buffers. */
size_t gsgen_knn_workspace_bytes(uint32_t n_points, uint32_t K);
int gsgen_knn(const float *points, uint32_t n_points, uint32_t K, float *dist2, int32_t *idx, void *workspace,
              size_t workspace_bytes, gsgen_stream_t stream);

/* The same search for a query set of its own: queries [n_queries,3] fp32, taken in the caller's order.  Row q of dist2 / idx
 * [n_queries,K] lists the K nearest `points` to queries[q] in ascending (dist2, index) order, dist2 = dx*dx + dy*dy + dz*dz with
 * d = p_j - q evaluated left to right (an fp32 brute force reproduces every bit).  A non-finite point is nobody's neighbour; a
 * non-finite query's row is (-1, +inf), and so is the tail of a row short of K finite points.  K in 1..32 (else
 * GSGEN_EUNSUPPORTED); n_points == 0, K > n_points or a null pointer: GSGEN_EINVAL; n_queries == 0: 0 (success), nothing enqueued.
 * The index over `points` is rebuilt by every call (the workspace holds it: gsgen_knn_query_workspace_bytes).  Launch shapes
 * depend on (n_points, n_queries, K) alone; no host synchronisation, no allocation: capturable. */
size_t gsgen_knn_query_workspace_bytes(uint32_t n_points, uint32_t n_queries, uint32_t K);
int gsgen_knn_query(const float *points, uint32_t n_points, const float *queries, uint32_t n_queries, uint32_t K, float *dist2,
                    int32_t *idx, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* The density lattice of the mesh export (utils/export.py:66-120, get_density_val_grid_from_ckpt), fused with the search:
 * out[(ix*ny + iy)*nz + iz] = sum over the kept neighbours j of opacity_j * exp(-0.5 * d^T Sigma_j^-1 d),
 * d = (axis_x[ix], axis_y[iy], axis_z[iz]) - mean_j.  The neighbours are the K + skip_nearest nearest centres of the lattice
 * point (order and ties as gsgen_knn_query) with the first skip_nearest (0 or 1) dropped -- the reference searches K + 1 and
 * drops column 0, so 1 reproduces it.  A missing neighbour (fewer finite centres than asked for, a non-finite lattice
 * coordinate) contributes 0.  Sigma_j^-1 = R diag(1 / scale^2) R^T in closed form from qvec [N,4] (w first, normalised as the
 * projection does) and the ACTIVATED scale [N,3]; opacity [N] activated.  K + skip_nearest in 1..32 (else GSGEN_EUNSUPPORTED);
 * N == 0, K + skip_nearest > N, skip_nearest > 1 or a null pointer: GSGEN_EINVAL; an empty lattice: 0 (success).
 * workspace: gsgen_density_grid_workspace_bytes(N, K), for either value of skip_nearest.  Capturable like gsgen_knn. */
size_t gsgen_density_grid_workspace_bytes(uint32_t n_points, uint32_t K);
int gsgen_density_grid(const float *mean, const float *qvec, const float *scale, const float *opacity, uint32_t N,
                       const float *axis_x, const float *axis_y, const float *axis_z, uint32_t nx, uint32_t ny, uint32_t nz,
                       uint32_t K, uint32_t skip_nearest, float *out, void *workspace, size_t workspace_bytes,
                       gsgen_stream_t stream);

/* The same field at Q points of the caller's own (mesh vertices: normals and colours), one fused search-and-sum launch, queries in
 * the caller's order.  With the list of the Ks = K + skip_nearest nearest centres of a point q, d = q - mean_j,
 * t_j = opacity_j * exp(-0.5 * d^T Sigma_j^-1 d) evaluated as gsgen_density_grid evaluates it:
 *   density [Q]    sum of t_j over list entries skip_nearest .. Ks-1: bit-identical to gsgen_density_grid at the same coordinates;
 *   grad    [Q,3]  the gradient of that sum in q with the neighbour set held fixed: sum of -(t_j * (Sigma_j^-1 d));
 *   rgb     [Q,3]  sum of t_j color_j / sum of t_j over ALL Ks entries (the nearest centre counts even where the field drops it);
 *                  where the denominator is below 2^-126, the colour of the nearest centre, copied.  color [N,3], any range.
 * Any of density, grad, rgb may be NULL (not computed; the others' bits do not depend on it); rgb without color: GSGEN_EINVAL.
 * A non-finite point writes 0 everywhere; a missing neighbour contributes nothing.  The gradient's Sigma_j^-1 is the same closed
 * form evaluated in fp64 and rounded to fp32 once (the workspace holds it behind the lattice's layout:
 * gsgen_density_points_workspace_bytes(N, K), for either value of skip_nearest); the terms t_j take the lattice's own record.
 * Other argument rules and capturability as gsgen_density_grid; Q == 0: 0 (success), nothing enqueued. */
size_t gsgen_density_points_workspace_bytes(uint32_t n_points, uint32_t K);
int gsgen_density_points(const float *mean, const float *qvec, const float *scale, const float *opacity, const float *color,
                         uint32_t N, const float *points, uint32_t Q, uint32_t K, uint32_t skip_nearest, float *density,
                         float *grad, float *rgb, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* Point-cloud normals and local frames (pytorch3d's estimate_pointcloud_local_coord_frames, as utils/ops.py:62-72 calls it), fused
 * with the self search: the neighbourhood of point i is row i of gsgen_knn for the same K (the point itself included), never written
 * to memory.  In fp32, in this order: d_k = p_jk - p_i; m = (sum_k d_k) / K; c_k = d_k - m; C = (sum_k c_k c_k^T) / K; the eigen-
 * decomposition of C by cyclic Jacobi, eigenvalues ascending.
 *   normals   [n_points,3]    the unit eigenvector of the smallest eigenvalue;
 *   curvature [n_points,3]    the eigenvalues, ascending;
 *   frames    [n_points,3,3]  row-major, columns n, y, z (z: the largest eigenvalue): frames[i][r][0] == normals[i][r].
 * disambiguate != 0: n and z point to the side where at least K/2 of the neighbours lie (pytorch3d's rule); where neither side
 * reaches K/2, to the side of the positive sum of projections, and failing that the first non-zero component is positive (pytorch3d's
 * result depends on its solver's sign there); y = n x z.  disambiguate == 0: the solver's columns, each with its first non-zero
 * component positive.  A non-finite point and a row short of K finite neighbours write zeros; a rank-deficient covariance still
 * writes a unit normal and an orthonormal frame, the same bits on every run.  Any of the three outputs may be NULL (not written;
 * the others' bits do not depend on it); all three NULL: GSGEN_EINVAL.  K in 3..64 (else GSGEN_EUNSUPPORTED, workspace size 0);
 * n_points == 0, K >= n_points (pytorch3d requires a cloud larger than the neighbourhood) or a null points / workspace:
 * GSGEN_EINVAL; a short workspace: GSGEN_EWORKSPACE.  Capturable like gsgen_knn. */
size_t gsgen_point_normals_workspace_bytes(uint32_t n_points, uint32_t K);
int gsgen_point_normals(const float *points, uint32_t n_points, uint32_t K, uint32_t disambiguate, float *normals, float *curvature,
                        float *frames, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* ---- exact farthest point sampling (gsgen_amd/csrc/fps.hip) ------------------------------------------------------
 * replaces pytorch3d's sample_farthest_points as utils/ops.py:76-100 calls it (guidance/point_e.py:120-127, :169-179).
 * points fp32, n_starts clouds of [n_points, dim] rows, cloud_stride floats between the clouds of consecutive starts (0: every
 * start samples the same cloud).  lengths: device int32[n_starts] (cloud b is its first lengths[b] rows) or null; start_idx:
 * device int32[n_starts], read by the kernel; idx_out: device int32[n_starts, K].
 * Row b: idx[0] = start_idx[b] (the lowest-index finite point when that is out of range or not finite); m[p] = +inf; after pick s,
 * m[p] = min(m[p], d2(p, s)), d2 = sum over the coordinates of (p_c - s_c)^2 left to right in fp32 (an fp32 loop reproduces every
 * bit); the next pick is the point of the largest m, ties to the lowest index.  A point with a NaN / Inf coordinate is never
 * picked; entries past the number of pickable points are -1.
 * method: 0 auto, 1 brute (dim 3 or 6), 2 bucket-pruned (dim 3; same result).  Another dim, method or pair: GSGEN_EUNSUPPORTED
 * (workspace size 0).  K == 0, n_points == 0, n_starts == 0, a null pointer or a workspace smaller than
 * gsgen_fps_workspace_bytes of the same sizes and method: GSGEN_EINVAL.  Launch shapes depend on the sizes alone; no allocation, no
 * host synchronisation: capturable, and a replay samples from the starts and point values then in the buffers. */
size_t gsgen_fps_workspace_bytes(uint32_t n_points, uint32_t dim, uint32_t n_starts, uint32_t K, int method);
int gsgen_fps(const float *points, uint32_t n_points, uint32_t dim, size_t cloud_stride, const int32_t *lengths,
              const int32_t *start_idx, uint32_t n_starts, uint32_t K, int32_t *idx_out, void *workspace, size_t workspace_bytes,
              int method, gsgen_stream_t stream);

/* ---- fused SSIM + L1 / L2 image loss (gsgen_amd/csrc/loss.hip) --------------------------------------------------------
 * replaces utils/loss.py:7-47: ssim_weight * kornia.losses.ssim_loss(out, gt, ws, "mean") + (1 - ssim_weight) * {mse | l1}(out, gt).
 * out, gt: device fp32 [B,H,W,C], channels last, contiguous.  With p = (ws - 1) / 2, g[i] = exp(-(i - ws/2)^2 / 4.5) / sum and
 * filt(x) the per-channel correlation of x, reflect-padded by p (the edge sample is not repeated), with g (x) g:
 *   mu1 = filt(out), mu2 = filt(gt), s1 = filt(out^2) - mu1^2, s2 = filt(gt^2) - mu2^2, s12 = filt(out gt) - mu1 mu2,
 *   s = (2 mu1 mu2 + 1e-4)(2 s12 + 9e-4) / ((mu1^2 + mu2^2 + 1e-4)(s1 + s2 + 9e-4) + 1e-12),
 *   loss = ssim_weight * mean(clamp((1 - s) / 2, 0, 1)) + (1 - ssim_weight) * mean(base_kind 0: (out - gt)^2, 1: |out - gt|).
 * ws odd in 3..11 and C in {1, 3}: a larger window, another C or base_kind is GSGEN_EUNSUPPORTED; an even window, ws < 3, H or
 * W < p + 1 (torch's own reflect limit) or a null pointer: GSGEN_EINVAL; a workspace smaller than the query's answer for the same
 * sizes: GSGEN_EWORKSPACE; a refused call enqueues nothing.  B * H * W == 0: 0 (success), nothing enqueued.
 * forward: loss_out device float[3] = the loss, its ssim term, its base term (the two unweighted means).  With want_grad it also
 *   saves three per-pixel derivative maps in the workspace (3 * B * H * W * C floats; gsgen_image_loss_workspace_bytes with
 *   want_grad = 1), which the backward reads: call it with the same images, sizes, weight and workspace.
 * backward: grad_out_image [B,H,W,C] = *grad_scale_dev * d loss / d out (overwritten; no gradient to gt).  The upstream scalar is
 *   read on the device.
 * Sums are reduced in a fixed order, no float atomics: loss and gradient are bit-identical from run to run.  Launch shapes depend
 * on the sizes alone, no allocation, no host synchronisation: capturable, and a replay sees the values then in the buffers. */
size_t gsgen_image_loss_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws, int want_grad);
int gsgen_image_loss_forward(const float *out, const float *gt, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws,
                             float ssim_weight, int base_kind, int want_grad, float *loss_out, void *workspace, size_t workspace_bytes,
                             gsgen_stream_t stream);
int gsgen_image_loss_backward(const float *out, const float *gt, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws,
                              float ssim_weight, int base_kind, const float *grad_scale_dev, float *grad_out_image, void *workspace,
                              size_t workspace_bytes, gsgen_stream_t stream);

/* ---- Pearson depth loss (gsgen_amd/csrc/depth_loss.hip) ---------------------------------------------------------------
 * replaces utils/loss.py:50-66: (1 / B) sum_b (1 - PearsonCorrCoef(nan_to_num(pred_b)[mask_b], gt_b[mask_b])), the loop over the
 * batch with a boolean gather per image.  pred: device fp32 [B][n_pixels], contiguous.  gt: fp32, image b at gt + b *
 * gt_image_stride (in elements); mask: uint8, non-zero = true, image b at mask + b * mask_image_stride, NULL = all true.  An
 * image stride of 0 shares one gt / one mask across the batch.  Per image, over the masked pixels (n of them), with
 * x = nan_to_num(pred) (NaN -> 0, +-Inf -> +-FLT_MAX) and y = gt as it is:
 *   xm = sum x / n, ym = sum y / n, Sxx = sum (x - xm)^2, Syy = sum (y - ym)^2, Sxy = sum (x - xm)(y - ym),
 *   r = clamp(Sxy / sqrt(Sxx Syy), -1, 1),  loss = (1 / B) sum_b (1 - r_b).
 * A DEGENERATE image -- n < 2, all masked x equal, or all masked y equal (decided exactly, from the minimum and maximum) -- is
 * where the reference returns NaN; here it contributes 1 (r = 0) and a zero gradient.  A NaN in gt under the mask is not
 * sanitised: the loss is NaN.
 * forward: loss_out device float[1 + B] = the loss, then r_b per image (NaN for a degenerate image).  It saves the per-image
 *   moments in the workspace, which the backward reads: call it with the same arrays, sizes and workspace.
 * backward: grad_pred [B][n_pixels] and grad_gt (laid out as gt is) = *grad_scale_dev * d loss / d pred, d loss / d gt; either may be
 *   NULL; both are overwritten, with zeros outside the mask, for a degenerate image, where the clamp is active and (grad_pred
 *   only) where pred was not finite.  The upstream scalar is read on the device.
 * B > 65535: GSGEN_EUNSUPPORTED (the workspace query answers 0); a null pred, gt, loss_out, grad_scale_dev or workspace, or a
 * grad_gt with gt_image_stride == 0 and B > 1: GSGEN_EINVAL; a workspace smaller than the query's answer: GSGEN_EWORKSPACE; a
 * refused call enqueues nothing.  B * n_pixels == 0: 0 (success), nothing enqueued.  The workspace (80 bytes per 4096 pixels of an
 * image + 48 per image) may be dirty and unaligned: there is no fill launch.  Moments are summed in fp64 about a value of the data
 * and merged in a fixed order, no float atomics: loss and gradients are bit-identical from run to run.  Two launches forward, one
 * backward, their shapes from B and n_pixels alone, no allocation, no host synchronisation: capturable, and a replay sees the
 * values then in the buffers, the mask included. */
size_t gsgen_depth_loss_workspace_bytes(uint32_t B, uint32_t n_pixels);
int gsgen_depth_loss_forward(const float *pred, const float *gt, size_t gt_image_stride, const uint8_t *mask, size_t mask_image_stride,
                             uint32_t B, uint32_t n_pixels, float *loss_out, void *workspace, size_t workspace_bytes,
                             gsgen_stream_t stream);
int gsgen_depth_loss_backward(const float *pred, const float *gt, size_t gt_image_stride, const uint8_t *mask, size_t mask_image_stride,
                              uint32_t B, uint32_t n_pixels, const float *grad_scale_dev, float *grad_pred, float *grad_gt,
                              void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* ---- map regularisers: sparsity, opague and z_var (gsgen_amd/csrc/map_loss.hip) -----------------------------------------
 * replaces trainer.py:345-382: the three regularisers of the text-to-3D step on the rendered maps.  opacity, z_var: device fp32
 * [n_pixels], contiguous, at any 4-byte alignment (n_pixels = B H W: pixels meet only in the means).  Per pixel, in fp32, with
 * lo = (float)1e-3, hi = (float)(1.0 - 1e-3), c = clamp(opacity, lo, hi) (a NaN stays), in = lo <= opacity <= hi, m = c > 0.5f:
 *   sparsity s = sqrtf(opacity^2 + 0.01f);  opague e = -(c logf(c) + (1 - c) logf(1 - c));  z_var z = (z_var / c) * m (a product:
 *   a non-finite z_var under m == 0 gives NaN, as in torch);  T_k = the mean over the pixels;  total = w_s T_s + w_o T_o + w_z T_z.
 *   d s / d opacity = opacity / s;  d e / d opacity = in (logf(1 - c) - logf(c));  d z / d z_var = m / c;  d z / d opacity =
 *   -in m z_var / c^2 (the clamp passes the gradient on its bounds, as torch.clamp does).
 * terms_mask: bit 0 sparsity, bit 1 opague, bit 2 z_var; a term whose bit is clear is not evaluated (no log without bit 1, z_var
 *   not read without bit 2), reports 0 and adds nothing to total or to the gradients.  z_var may be NULL without bit 2.
 * The weights (w_s, w_o, w_z) are weights_host[3], read by the call, or -- when weights_dev is not NULL -- float[3] in device memory
 *   read by the kernels: a captured forward + backward replays with the weights then in that buffer.  One of the two is required.
 * forward: loss_out device float[4] = total, T_s, T_o, T_z.  Two launches.
 * backward: grad_opacity, grad_z_var [n_pixels] = *grad_scale_dev * d total / d opacity, d total / d z_var; either may be NULL; both
 *   are overwritten (grad_z_var with zeros without bit 2).  It recomputes from the maps: nothing of the forward's is read, the
 *   workspace is only checked.  The upstream scalar is read on the device.  One launch.
 * A null opacity, loss_out, grad_scale_dev or workspace, neither weights_host nor weights_dev, a bit above 2 in terms_mask, or bit 2
 * without z_var: GSGEN_EINVAL; a workspace smaller than the query's answer: GSGEN_EWORKSPACE; a refused call enqueues nothing.
 * n_pixels == 0: 0 (success), nothing enqueued.  The workspace (24 bytes per 2048 pixels) may be dirty and unaligned: there is no
 * fill launch.  Per-pixel values are summed in fp64 in a fixed order, no float atomics: loss and gradients are bit-identical from
 * run to run and do not depend on the alignment of the maps.  Launch shapes from n_pixels alone, no allocation, no host
 * synchronisation: capturable, and a replay sees the values then in the buffers. */
size_t gsgen_map_loss_workspace_bytes(uint32_t n_pixels);
int gsgen_map_loss_forward(const float *opacity, const float *z_var, uint32_t n_pixels, uint32_t terms_mask, const float *weights_host,
                           const float *weights_dev, float *loss_out, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);
int gsgen_map_loss_backward(const float *opacity, const float *z_var, uint32_t n_pixels, uint32_t terms_mask, const float *weights_host,
                            const float *weights_dev, const float *grad_scale_dev, float *grad_opacity, float *grad_z_var,
                            void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* ---- marching cubes over a dense lattice (gsgen_amd/csrc/marching_cubes.hip) -------------------------------------------
 * replaces the PyMCubes call of utils/export.py:123-155.  grid: device fp32 [X][Y][Z], x slowest, contiguous (what
 * gsgen_density_grid writes).  A lattice point is inside iff grid - thresh > 0 in fp32 (NaN: outside), the convention of the
 * reference's own shap_e/rendering/mc.py; PyMCubes' tie-breaking at grid == thresh and its triangle order are not reproduced.
 * verts [verts_capacity,3] fp32 in lattice index coordinates: one vertex per lattice edge whose end points differ in insideness,
 *   all x-edges first, then y-, then z-edges, each in the raster order of the edge's lower point; with s1, s2 the values of
 *   grid - thresh at the lower point p1 and at p2 = p1 + e_axis:  t = s1 / (s1 - s2), v = t * p2 + (1 - t) * p1, fp32, unfused.
 * tris [tris_capacity,3] int32 vertex ids, 0..5 triangles per cube in cube raster order, normals from inside to outside.
 * counts: device uint32[3] = {V, F, overflow}: always the true numbers of vertices and triangles; overflow = 1 when V >
 *   verts_capacity or F > tris_capacity.  Then nothing is written past a capacity and the rows that fit are valid, but a written
 *   triangle may name a vertex that was dropped: check the flag.  Capacities 0 (the pointers may then be NULL) only count.
 * Any of X, Y, Z < 2 or X * Y * Z > 2^30: GSGEN_EUNSUPPORTED (the workspace query answers 0); a null grid, counts or workspace, a
 * null output with a non-zero capacity, a capacity above 2^31 - 1: GSGEN_EINVAL; a workspace smaller than the query's answer:
 * GSGEN_EWORKSPACE; a refused call enqueues nothing.  The workspace (4 bytes per lattice point + 32 per 1024 points) may be
 * dirty and unaligned.  No atomics, no allocation, no host synchronisation, launch shapes from X, Y, Z alone: capturable, and the
 * output is bit-identical from run to run.  F < 2^32 is assumed. */
size_t gsgen_marching_cubes_workspace_bytes(uint32_t X, uint32_t Y, uint32_t Z);
int gsgen_marching_cubes(const float *grid, uint32_t X, uint32_t Y, uint32_t Z, float thresh, float *verts, uint32_t verts_capacity,
                         int32_t *tris, uint32_t tris_capacity, uint32_t *counts, void *workspace, size_t workspace_bytes,
                         gsgen_stream_t stream);

/* ---- learned MLP background, fused with its composite (gsgen_amd/csrc/background.hip) -----------------------------------
 * replaces gs/backgrounds.py:88-114 (tcnn.NetworkWithInputEncoding: SphericalHarmonics degree 3 -> FullyFusedMLP ReLU 16 x 2) and
 * the composite of gs/renderer.py:1182.  DESIGN.md ("MLP background") has the definition, a reading of tinycudann that no reference
 * run pins.  Per pixel p = (b, y, x) of a [B][H][W] batch, in fp32:
 *   d = R_b ((x - cx) / fx, (y - cy) / fy, 1), e = 2 d - 1, u = (the 9 SH terms of degree < 3 at e, then seven ones),
 *   h1 = relu(W0 u), h2 = relu(W1 h1), o = (W2 h2)[0..2], bg = nan_to_num(sigmoid(o))  (a NaN becomes 0).
 * params: device float[768] = W0 | W1 | W2, each [16 out][16 in] row-major; rows 3..15 of W2 are never read.
 * Directions come from ONE of: cams -- per-view camera blocks in device memory, view b at cams + b * cam_stride_bytes (a multiple
 *   of 4, at least 64), floats 0..11 the c2w rows, 12..15 fx fy cx cy: what gsgen_pack_camera writes (BatchRenderer's blocks are
 *   272 bytes apart; a stand-alone caller may pack [B][16]); or dirs -- device float[B H W][3], used as d.  The other is NULL.
 * forward: out [B][H][W][3] = bg, or rgb_in + (1 - opacity) * bg when rgb_in [B][H][W][3] and opacity [B][H][W] are given (both
 *   or neither).  One launch.
 * backward: recomputes the forward per pixel (nothing per-pixel was saved).  grad_out [B][H][W][3] is the upstream gradient of
 *   out, read on the device.  grad_params float[768] is overwritten; the entries of W2's rows 3..15 are exactly 0.  With opacity
 *   given (the composite form) the background's gradient carries the factor (1 - opacity), and grad_opacity [B][H][W] (optional)
 *   = -sum_c grad_out_c bg_c.  The gradient of rgb_in is grad_out itself.  A pixel whose o is not finite contributes nothing to
 *   grad_params.  Two launches: per-workgroup partial sums on the exact fp32 MFMA, then a fixed-order sum; no float atomics, so
 *   the result is bit-identical from run to run.
 * B * H * W > 2^31: GSGEN_EUNSUPPORTED (the workspace query answers 0); a null params / out / grad_out / grad_params / workspace,
 * both or neither of cams and dirs, a bad cam_stride_bytes, rgb_in without opacity or the reverse, grad_opacity without opacity:
 * GSGEN_EINVAL; a workspace smaller than the query's answer: GSGEN_EWORKSPACE; a refused call enqueues nothing.  B * H * W == 0: 0
 * (success), nothing enqueued.  The workspace (3 KB per backward workgroup, at most 1024 of them) may be dirty and unaligned.  No
 * allocation, no host synchronisation, launch shapes from B, H, W alone: capturable, and a replay reads the parameters, camera
 * blocks and gradients then in the buffers. */
size_t gsgen_mlp_background_workspace_bytes(uint32_t B, uint32_t H, uint32_t W);
int gsgen_mlp_background_forward(const float *params, const void *cams, size_t cam_stride_bytes, const float *dirs, uint32_t B,
                                 uint32_t H, uint32_t W, const float *rgb_in, const float *opacity, float *out, gsgen_stream_t stream);
int gsgen_mlp_background_backward(const float *params, const void *cams, size_t cam_stride_bytes, const float *dirs, uint32_t B,
                                  uint32_t H, uint32_t W, const float *opacity, const float *grad_out, float *grad_params,
                                  float *grad_opacity, void *workspace, size_t workspace_bytes, gsgen_stream_t stream);

/* ---- triangle mesh -> evenly spaced point cloud (gsgen_amd/csrc/mesh_sample.hip) ------------------------------------------
 * replaces trimesh's sample_surface / remove_close / sample_surface_even under utils/mesh.py:52-69.  DESIGN.md ("Mesh sampling")
 * has the definitions.
 * gsgen_mesh_sample: verts [V][3] float, tris [F][3] int32, uniforms [M][3] float in [0, 1) = (u_face, r1, r2), all on the device.
 *   Face weight = 0.5 |(v1 - v0) x (v2 - v0)| in fp64; 0 for a zero area, a non-finite vertex or a vertex index outside [0, V).
 *   Sample m takes the first face i with cum[i] >= (double)u_face * total and weight > 0 (cum: the inclusive fp64 scan of the
 *   weights), flips (r1, r2) to (1 - r1, 1 - r2) where r1 + r2 > 1, and writes, each where the pointer is not NULL:
 *   points [M][3] = v0 + ((v1 - v0) r1 + (v2 - v0) r2), face_index [M], barycentric [M][2] = (r1, r2) after the flip, attr_out
 *   [M][A] from attributes [V][A] in the same form (A in 1..8; A = 0 with attributes = attr_out = NULL), normals [M][3] = the
 *   face's unit normal.  status (optional, 8-byte aligned, 16 bytes): uint32 bad_faces (faces with an index out of range),
 *   uint32 zero_area_flag, double total area.  Total area 0: every output row is NaN, face_index -1, zero_area_flag 1.
 *   A above 8, attributes without A or the reverse, a misaligned status, a null tris / workspace / verts / uniforms that is
 *   needed: GSGEN_EINVAL; a short workspace: GSGEN_EWORKSPACE.  F == 0, or M == 0 without a status block: 0, nothing enqueued;
 *   M == 0 with one: the weights and the scan alone (how the area is read).  The workspace (8 bytes per face and a little) may
 *   be dirty and unaligned.
 * gsgen_remove_close_init / _rounds: points [N][3]; keep [N] bytes.  Point i is kept iff no kept j < i has
 *   (dx dx + dy dy) + dz dz <= r r in fp32; a non-finite point is removed and is nobody's neighbour.  init builds the grid, sorts
 *   the points by cell and resets the state and keep[] (all 0); rounds enqueues n_rounds decision rounds (one launch each; keep[i]
 *   becomes 1 when i is decided kept) and then writes the number of points the last of them left undecided to *remaining
 *   (optional; n_rounds = 0: the count as it stands); a round that finds nothing undecided returns at once.  The same N, radius,
 *   keep and workspace go to init and to every rounds call after it; keep[] is final once *remaining is 0.  radius < 0 or NaN:
 *   GSGEN_EINVAL; a short workspace: GSGEN_EWORKSPACE; N == 0: 0, nothing enqueued.  The workspace (about 33 bytes per point) may
 *   start at any alignment.
 * Nothing here allocates or synchronises with the host; launch shapes depend on the sizes alone. */
size_t gsgen_mesh_sample_workspace_bytes(uint32_t n_faces);
int gsgen_mesh_sample(const float *verts, uint32_t n_verts, const int32_t *tris, uint32_t n_faces, const float *uniforms,
                      uint32_t n_samples, const float *attributes, uint32_t n_attr, float *points, int32_t *face_index,
                      float *barycentric, float *attr_out, float *normals, void *status, void *workspace, size_t workspace_bytes,
                      gsgen_stream_t stream);
size_t gsgen_remove_close_workspace_bytes(uint32_t n_points);
int gsgen_remove_close_init(const float *points, uint32_t n_points, float radius, uint8_t *keep, void *workspace,
                            size_t workspace_bytes, gsgen_stream_t stream);
int gsgen_remove_close_rounds(uint32_t n_rounds, uint32_t n_points, float radius, uint8_t *keep, uint32_t *remaining, void *workspace,
                              size_t workspace_bytes, gsgen_stream_t stream);

/* ---- guidance seam: the guidance's input image and the SDS loss (gsgen_amd/csrc/guidance_seam.hip) ---------------------------
 * replaces the torch sequences between the rendered batch and the diffusion guidance (guidance/stable_diffusion.py:274-312 and
 * its siblings).  DESIGN.md ("Guidance seam") has the definitions.
 * Guidance input: x device fp32 [B][H][W][C] channels last, C in {1, 3} -> out = scale * bilinear(x) + shift at OH x OW, torch's
 *   upsample_bilinear2d map with align_corners=False and no antialiasing in fp32, the affine applied once after the interpolation.
 *   out is planar [B][C][OH][OW] (out_planar != 0) or channels last [B][OH][OW][C], fp16 rounded to nearest even (out_half != 0) or
 *   fp32; with C == 1 the two layouts are one.
 *   The workspace holds the per-axis tables of the (H, W, OH, OW) quadruple: (i0, l1) per output index, [o_begin, o_end) per input
 *   index.  forward with build_tables != 0 writes them first (one tiny launch; the workspace may arrive dirty and unaligned); with
 *   build_tables == 0 it reads what an earlier forward with the same sizes and the same workspace address wrote, so a caller may
 *   keep one workspace per quadruple.  backward always reads them: call it with the workspace a forward filled.
 *   backward: grad_out in the layout grad_planar names, fp16 (grad_half != 0) or fp32 -> grad_x [B][H][W][C] fp32, overwritten: a
 *   gather, one lane per input pixel, summed output row ascending then output column ascending in fp32 with the forward's own
 *   weights (its exact adjoint); an input pixel no output read is written as an exact zero.  No float atomics, no fill.
 * SDS loss: grad device fp32 [B][n] -> g' = clamp(nan_to_num(grad), -clip, clip) (NaN -> 0, +-Inf -> +-FLT_MAX; the clamp only with
 *   use_clip != 0).  forward: loss_out device float[2 + B] = {0.5 sum g'^2 / B, sqrt(sum g'^2), 0.5 sum_b g'^2 per image}, sums in
 *   fp64 in a fixed order, and g' / B saved in the workspace.  The value does not depend on latents, so they are not passed.
 *   backward: grad_latents [B][n] = *grad_scale_dev * g' / B from the workspace the forward filled; the upstream scalar is read on
 *   the device.  Two launches forward, one backward.
 * A zero size or a null pointer (or a negative or NaN clip with use_clip): GSGEN_EINVAL; C not in {1, 3}, an image side above
 * 65536, B > 65535 (SDS) or a launch grid past 2^31 - 1 workgroups: GSGEN_EUNSUPPORTED (the workspace queries answer 0 for
 * both); a workspace smaller than the query's answer: GSGEN_EWORKSPACE; a refused call enqueues nothing.  No allocation, no host
 * synchronisation, launch shapes from the sizes alone: capturable, and a replay sees the values then in the buffers.  Everything
 * is bit-identical from run to run. */
size_t gsgen_guidance_input_workspace_bytes(uint32_t H, uint32_t W, uint32_t OH, uint32_t OW);
int gsgen_guidance_input_forward(const float *x, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t OH, uint32_t OW, float scale,
                                 float shift, int out_half, int out_planar, void *out, int build_tables, void *workspace,
                                 size_t workspace_bytes, gsgen_stream_t stream);
int gsgen_guidance_input_backward(const void *grad_out, int grad_half, int grad_planar, uint32_t B, uint32_t H, uint32_t W, uint32_t C,
                                  uint32_t OH, uint32_t OW, float scale, float *grad_x, void *workspace, size_t workspace_bytes,
                                  gsgen_stream_t stream);
size_t gsgen_sds_loss_workspace_bytes(uint32_t B, uint32_t n);
int gsgen_sds_loss_forward(const float *grad, uint32_t B, uint32_t n, int use_clip, float clip, float *loss_out, void *workspace,
                           size_t workspace_bytes, gsgen_stream_t stream);
int gsgen_sds_loss_backward(uint32_t B, uint32_t n, const float *grad_scale_dev, float *grad_latents, void *workspace,
                            size_t workspace_bytes, gsgen_stream_t stream);

/* Self test of the wave64 cross-lane reduce-scatter used by the backward (tests only):
 * in [64 lanes, P components]; out[0..64) = per-lane result, out[64..128) = the component index that
 * lane owns (-1: duplicate holder); P in {8,16,32,64}. */
int gsgen_selftest_reduce_scatter(uint32_t P, const float *in, float *out, gsgen_stream_t stream);

/* Self test of the separable 16-component reduce-scatter of the polynomial SH backward (tests only): in [64 lanes, 16 components]
 * (class k = lane / 16 keeps components 4 k .. 4 k + 3 = v0 .. v3), u [64 lanes] (equal for lanes that agree modulo 16);
 * out[0..64) = per-lane result, out[64..128) = the slot 8 * class + slot that lane owns (-1: none: second holder or a dead slot),
 * out[128..192) = the slot the lane's result belongs to.  Slots of classes 0..2: v0, v1, u v0, v2, u v1, u^2 v0, v3, -; of class 3:
 * v0, v1, 0, v2, 0, 0, v3, - (the kernel pads v3). */
int gsgen_selftest_reduce_scatter_sep16(const float *in, const float *u, float *out, gsgen_stream_t stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GSGEN_HIP_H */
