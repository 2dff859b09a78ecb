/*
 * nicer_slam_amd.h -- C ABI of the MI355X-native NICER-SLAM render core (libnicer_slam_amd.so).
 *
 * Plain pointers and sizes only; every buffer is DEVICE memory owned by the caller unless the
 * parameter name ends in `_host`.  Nothing is allocated or kept between calls.  All launches are
 * asynchronous on `stream` (a hipStream_t; NULL = the legacy default stream, which is what the
 * reference launches on).  Every entry point returns 0 (NSA_OK) or an NSA_E* code; the text the
 * reference would have thrown for that condition is available from nsa_strerror().
 *
 * Section 1 replaces, one for one, the three functions of the reference's native module
 * (reference: code/hashencoder/src/hashencoder.h:13-15, bound at code/hashencoder/src/bindings.cpp:5-7,
 *  implemented at code/hashencoder/src/hashencoder.cu:758-854).  Differences from that interface:
 *   - raw device pointers + an explicit stream instead of at::Tensor (the tensor checks of
 *     hashencoder.cu:759-775 live in the thin binding, nicer_slam_amd/hashencoder/backend.py);
 *   - `offsets_host` is a HOST copy of the int32 offsets tensor (the per-level geometry is derived
 *     on the host and passed as kernel arguments, so the device never calls exp2f/ceil);
 *   - float32 only (the reference also dispatches half/double; it never runs them);
 *   - an int status instead of a C++ exception.
 * Layouts are the reference's: inputs[B,D] in [0,1]; embeddings[rows,C]; outputs[L,B,C] (level-major);
 * dy_dx[B,L,D,C]; grad[L,B,C]; grad_embeddings/grad2_embeddings[rows,C] are ACCUMULATED INTO with
 * float atomics (caller pre-zeroes, as hashgrid.py:84-85,117-118 does); grad_inputs[B,D] and
 * grad_grad[L,B,C] are overwritten.
 */
#ifndef NICER_SLAM_AMD_H
#define NICER_SLAM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSA_OK 0
#define NSA_EUNSUPPORTED_C 1   /* "GridEncoding: C must be 1, 2, 4, or 8." (hashencoder.cu:637,652,...) */
#define NSA_ETOO_MANY_LEVELS 2 /* more than NSA_MAX_LEVELS levels */
#define NSA_ELAUNCH 3          /* hipGetLastError() != hipSuccess after a launch */
#define NSA_EBADARG 4          /* null pointer / inconsistent sizes */
#define NSA_EUNSUPPORTED_NET 5 /* fused core: network shape outside the compiled set */
#define NSA_EMESH_TOO_LARGE 6  /* marching cubes: a vertex or face total does not fit int32 */

#define NSA_MAX_LEVELS 32

typedef void *nsa_stream_t; /* hipStream_t */

const char *nsa_strerror(int code);
int nsa_version(void);

/* ---- Section 1: hash/dense multi-resolution grid encoder (reference hashencoder.h:13-15) ---- */

/* replaces hash_encode_forward (hashencoder.cu:758-781 -> kernel_grid :131-283).
 * dy_dx may be NULL when calc_grad_inputs == 0. */
int nsa_hash_encode_forward(const float *inputs, const float *embeddings, const int32_t *offsets_host,
                            float *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                            uint32_t H, int calc_grad_inputs, float *dy_dx, nsa_stream_t stream);

/* replaces hash_encode_backward (hashencoder.cu:783-813 -> kernel_grid_backward :286-373 and
 * kernel_input_backward :376-402).  grad_embeddings may be NULL to skip the table scatter
 * (extension: used when the table does not require grad). */
int nsa_hash_encode_backward(const float *grad, const float *inputs, const float *embeddings,
                             const int32_t *offsets_host, float *grad_embeddings, uint32_t B, uint32_t D,
                             uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                             const float *dy_dx, float *grad_inputs, nsa_stream_t stream);

/* replaces hash_encode_second_backward (hashencoder.cu:816-854 -> kernel_grid_second_backward_grad
 * :405-458 and kernel_grid_second_backward_embedding :461-625).  C == 1 is rejected like the
 * reference (:708-714).  grad2_embeddings may be NULL to skip the table scatter (extension). */
int nsa_hash_encode_second_backward(const float *grad, const float *inputs, const float *embeddings,
                                    const int32_t *offsets_host, uint32_t B, uint32_t D, uint32_t C,
                                    uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                    const float *dy_dx, const float *grad_grad_inputs, float *grad_grad,
                                    float *grad2_embeddings, nsa_stream_t stream);

/* ---- Section 2: fused render core (no native counterpart in the reference: these replace the PyTorch-level
 * functions named at each entry point; rays, samples and per-point quantities stay in HBM between them) ---- */

/* One multi-resolution grid + the MLP that consumes it. */
typedef struct nsa_grid {
    const float *table;          /* embeddings[rows, C] (device)                                   */
    const int32_t *offsets_host; /* [L+1] (host)                                                   */
    uint32_t L, C;               /* levels, features per level                                     */
    float S;                     /* log2(per_level_scale)                                          */
    uint32_t H;                  /* base resolution                                                */
    float divide_factor;         /* x is divided by this before the [-1,1] -> [0,1] map            */
    uint32_t n_hidden;           /* hidden layers of the attached MLP (coarse 1, fine 3)           */
    uint32_t precision;          /* GEMM operands of the attached MLP: 0 = fp32-faithful (the reference's precision; default:
                                  * two fp16 pieces per operand after a per-point power-of-two scale, or three exact bf16
                                  * pieces in a -DNSA_FORM=3 build, nsa_operand_form), 1 = plain bf16 operands with fp32 accumulation
                                  * (optional "bf16 MLP" mode of BASELINE configs 2/4; encoders, activations,
                                  * compositing and all reductions stay fp32)                       */
    uint32_t tile;               /* tiling of the SDF-network kernels and the matching packed-parameter layout: 16 = quad
                                  * tiling (16 points per wave, four lanes per point; pack_sdf_net4), 0 or 32 = 32-point
                                  * tiling (lane pair per point; pack_sdf_net).  Ignored by the colour network.          */
} nsa_grid_t;

/* Where the points of a per-point kernel come from: sample (pid % S) of ray (pid / S), x = o + z d -- or, when
 * `points` is non-NULL, an explicit list (eikonal samples). */
typedef struct nsa_points {
    const float *rays_o;  /* [R,3] */
    const float *rays_d;  /* [R,3] */
    const float *z_vals;  /* [R,S] */
    const float *points;  /* [P,3] or NULL */
    uint32_t P, S;        /* P = R*S in ray mode */
    const uint32_t *order; /* optional [P] launch order (a permutation): work item i processes point order[i].  Per-point
                            * arrays (sdf, grad, rgb, g_*) stay indexed by point; tile-indexed buffers (HL feature
                            * vectors, the colour save area, emission rows) are indexed by work item, consistently
                            * across the forward and backward entry points.  NULL = identity. */
} nsa_points_t;

/* Per-point feature vectors travel in "HL" layout (the MFMA register image): float index ((tile*32+q)*64+lane),
 * tile = point/32, sized ceil(P/32)*2048 floats; see csrc/mlp_common.hpp. */

/* One SDF network (coarse or fine) at P points: sdf, grad sdf (reverse pass, kept differentiable by
 * nsa_sdfnet_backward) and the 64-feature vector.  accumulate != 0 adds to sdf/grad/feat (the fine network on
 * top of the coarse one).  replaces ImplicitNetworkGrid.get_outputs / ImplicitNetworkGrid_COMBINE.get_outputs
 * (code/model/base_networks.py:34-40,208-221) incl. HashEncoder.forward and the positional encoding. */
int nsa_sdfnet_forward(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, int accumulate,
                       float *sdf, float *grad, float *feat_hl, nsa_stream_t stream);

/* Both networks of the COMBINE in one launch: what nsa_sdfnet_forward(coarse, accumulate 0) followed by
 * nsa_sdfnet_forward(fine, accumulate 1) leaves in sdf / grad / feat_hl, bit for bit, for the quad tiling (both descriptors
 * tile == 16 with their quad packs, the same precision).  Point, positional encoding, level geometry and outputs are handled
 * once; the coarse results stay in registers.  replaces ImplicitNetworkGrid_COMBINE.get_outputs
 * (code/model/base_networks.py:7-47) in the "fine" stage. */
int nsa_sdfnet_forward_pair(const nsa_points_t *pts, const nsa_grid_t *coarse, const nsa_grid_t *fine,
                            const float *packed_coarse, const float *packed_fine, float *sdf, float *grad, float *feat_hl,
                            nsa_stream_t stream);

/* Backward of the above for the DATA path: given d/d(sdf)[P], d/d(feat) (HL), d/d(grad sdf)[P,3] (any may be
 * NULL = zero) produce d/dx [P,3] -- value path + double backward through the reverse pass, with exactly the terms
 * of the reference graph (the grid-Hessian term is dropped, code/hashencoder/hashgrid.py:134). */
int nsa_sdfnet_backward(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *g_sdf,
                        const float *g_feat_hl, const float *g_grad, int accumulate, float *g_x,
                        nsa_stream_t stream);

/* Pixels -> rays for b images x n pixels: rays_o[b*n,3] = pose[:3,3], rays_d = (p - o)/|p - o|^2 (NOT unit length),
 * depth_scale[b*n] = z of the identity-pose direction.  replaces rend_util.get_camera_params + lift
 * (code/utils/rend_util.py:68-93,107-129), both calls of code/model/network.py:98-102. */
int nsa_rays_forward(const float *uv, const float *pose, const float *K, uint32_t b, uint32_t n, float *rays_o,
                     float *rays_d, float *depth_scale, nsa_stream_t stream);

/* nsa_rays_forward and the sampler's draws of the pass (nsa_draw: n_rand uniforms into t_rand, the n_extra picks of E into
 * extra_idx, no eikonal picks) in ONE launch -- the draw's workgroups ride beside the ray lifting.  Same rays, same draws. */
int nsa_rays_forward_draw(const float *uv, const float *pose, const float *K, uint32_t b, uint32_t n, float *rays_o,
                          float *rays_d, float *depth_scale, uint64_t *state, uint64_t n_rand, float *t_rand, uint32_t E,
                          uint32_t n_extra, uint32_t S, int32_t *extra_idx, nsa_stream_t stream);

/* Backward of the above to the camera-to-world matrices: g_pose[b,4,4] (overwritten; bottom row zero).  Deterministic: one
 * workgroup per image, fixed-order sums, no atomics. */
int nsa_rays_pose_backward(const float *uv, const float *pose, const float *K, uint32_t b, uint32_t n,
                           const float *g_rays_o, const float *g_rays_d, float *g_pose, nsa_stream_t stream);

/* Colour network at the composite points: rgb = sigmoid(MLP([x, PE4(view dir), grad sdf, feature, colour grid])).
 * replaces RenderingNetwork.forward, mode "idr" (code/model/base_networks.py:333-395).  `save` (optional,
 * ceil(P/32)*(4096 + 256) floats) receives what the backward needs: from the 1 GiB colour table the features + Jacobian (4096 floats per
 * 32-point tile), and of the MLP itself the ReLU masks of both hidden layers and the sigmoid outputs (256 floats per tile, behind the
 * ceil(P/32)*4096 block) -- the data-path backward (nsa_colour_backward, nsa_colour_coarse_backward) reads those instead of
 * recomputing the forward; the mapping backward (nsa_colour_backward_params) recomputes it (its activations are gradient operands). */
int nsa_colour_forward(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                       const float *feat_hl, float *rgb, float *save, nsa_stream_t stream);

/* nsa_colour_forward followed by nsa_composite_forward as two phases of ONE launch, under the conditions of
 * nsa_colour_forward_track below (ray samples in ray order, 128 per ray: a workgroup of the colour forward is one ray): weights,
 * rgb_values, depth, nmap, entropy as nsa_composite_forward leaves them.  Identical results. */
int nsa_colour_forward_composite(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                                 const float *feat_hl, float *rgb, float *save, const float *sdf, const float *voxels,
                                 uint32_t voxel_res, float *weights, float *rgb_values, float *depth, float *nmap,
                                 float *entropy, nsa_stream_t stream);

/* nsa_colour_forward followed by nsa_composite_track as two phases of ONE launch, for ray samples in ray order with 128 samples per
 * ray (P a multiple of 128, no launch order): a workgroup of the colour forward holds exactly one ray, and when its colours are stored
 * its first wave forms the ray's rendered colour, the L1 cotangent and the composite backward (arguments as for nsa_composite_track;
 * R = P / 128).  The same statements as the two kernels: identical results; the per-ray kernel's launch disappears into the tail of
 * the colour forward.  This entry leaves the 16 FEATURE slots per lane of `save` unwritten (the Jacobian, the ReLU masks and the outputs
 * are written): what follows it is the data-path backward; nsa_colour_backward_params needs a save area written by nsa_colour_forward
 * or nsa_colour_forward_composite. */
int nsa_colour_forward_track(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                             const float *feat_hl, float *rgb, float *save, const float *sdf, const float *voxels,
                             uint32_t voxel_res, const float *gt, uint32_t n_total, float *rgb_values, float *ray_loss,
                             float *g_sdf, float *g_rgb, float *g_grad, nsa_stream_t stream);

/* Data-path backward of the colour network: d/d(rgb)[P,3] -> d/d(feat) (HL, overwritten), d/d(grad sdf)[P,3]
 * (ADDED into g_grad), d/dx [P,3] and d/d(view dir) [P,3] (overwritten).  grid_grad = 0 reproduces
 * color_stage == "base" (grid feature detached, base_networks.py:337-339). */
int nsa_colour_backward(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                        const float *feat_hl, const float *save, const float *g_rgb, int grid_grad,
                        float *g_feat_hl, float *g_grad, float *g_x, float *g_dir, nsa_stream_t stream);

/* nsa_colour_backward followed by nsa_sdfnet_backward(coarse, accumulate 1) -- the coarse network in the 32-point tiling, the
 * tiles of the colour kernels -- as two phases of ONE launch: every wave runs the colour backward of its 32 points and then the
 * coarse SDF backward of the same points (g_sdf: d/d sdf from the composite; the feature and normal cotangents and the d/dx to
 * accumulate onto are what its first phase has just written).  The same statements as the two kernels: identical results.
 * For a tracking batch, where both kernels run only two rounds of waves, the input burst of a round is paid once. */
int nsa_colour_coarse_backward(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                               const float *feat_hl, const float *save, const float *g_rgb, int grid_grad, float *g_feat_hl,
                               float *g_grad, float *g_x, float *g_dir, const nsa_grid_t *coarse, const float *packed_coarse,
                               const float *g_sdf, nsa_stream_t stream);

/* Mapping-mode backward (parameter gradients): the same kernels as nsa_sdfnet_backward / nsa_colour_backward with two
 * more outputs; the data path is bit-identical to theirs except for the coarse SDF network in the 32-point tiling, whose MAP kernel
 * keeps the grid Jacobian in LDS where the plain one recomputes it from the corner gathers (same sums, another rounding order).
 * Replaces, for a mapping iteration, what torch.autograd does through ImplicitNetworkGrid / RenderingNetwork /
 * _hash_encode.backward / _hash_encode_second_backward (code/model/base_networks.py:195-221, 333-395;
 * code/hashencoder/hashgrid.py:64-141) for the trainable parameters of volsdf_train.py:150-173:
 *   g_table  gradient of the grid table (same shape as grid->table), ATOMICALLY ACCUMULATED (caller zeroes it):
 *            value path + (SDF grids) the table's share of the double backward through grad sdf; may be NULL.
 *   emit     [nsa_*_emit_rows()][emit_ld] per-point vectors, column = point index (emit_ld >= ceil(P/32)*32 -- the quad tiling writes 16-point tiles, so its padding starts at ceil(P/16)*16 --, columns
 *            of padding points are written as 0).  The weight gradients are GEMMs over these rows (row map: the
 *            SE_* / CE_* enums in csrc/render_sdfnet.hip, csrc/render_colour.hip; host side fused/mapping.py).
 *            SDF: nsa_sdfnet_emit_rows_nh(grid->n_hidden) rows (464 for the coarse network, 976 for the fine one, whose
 *            gradients the reference computes but never applies, volsdf_train.py:150-173); may be NULL. */
int nsa_sdfnet_backward_params(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *g_sdf,
                               const float *g_feat_hl, const float *g_grad, int accumulate, float *g_x, float *g_table,
                               float *emit, uint32_t emit_ld, nsa_stream_t stream);
int nsa_colour_backward_params(const nsa_points_t *pts, const nsa_grid_t *grid, const float *packed, const float *grad,
                               const float *feat_hl, const float *save, const float *g_rgb, int grid_grad,
                               float *g_feat_hl, float *g_grad, float *g_x, float *g_dir, float *g_table, float *emit,
                               uint32_t emit_ld, nsa_stream_t stream);
int nsa_sdfnet_emit_rows(void);                 /* one hidden layer (coarse network) */
int nsa_sdfnet_emit_rows_nh(uint32_t n_hidden); /* 1 or 3 hidden layers; -1 otherwise (32-point tiling) */
int nsa_sdfnet_emit_rows_tile(uint32_t n_hidden, uint32_t tile); /* the same for nsa_grid_t.tile = 16 / 32 */
int nsa_colour_emit_rows(void);

/* Per-ray SDF -> density -> alpha compositing.  replaces SLAMNetwork.volume_rendering (code/model/network.py:349-370)
 * + the composite sums of SLAMNetwork.forward (:147-151, 298, 338-342) + GridPredefineDensity (density.py:37-67).
 * Outputs weights[R,S], rgb_values[R,3], depth[R] (= sum w z / (sum w + 1e-8), before depth_scale),
 * nmap[R,3] (= sum w grad/(|grad|+1e-6), before the rotation by the pose), entropy[R] (= sum -w log(w+1e-4)). */
int nsa_composite_forward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf,
                          const float *rgb, const float *grad, const float *voxels, uint32_t voxel_res, uint32_t R,
                          uint32_t S, float *weights, float *rgb_values, float *depth, float *nmap, float *entropy,
                          nsa_stream_t stream);

/* Backward of the above: per-ray cotangents (any may be NULL) -> d/d(sdf)[R,S], d/d(rgb)[R,S,3], d/d(grad)[R,S,3]. */
int nsa_composite_backward(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf,
                           const float *rgb, const float *grad, const float *voxels, uint32_t voxel_res, uint32_t R,
                           uint32_t S, const float *g_rgb_values, const float *g_depth, const float *g_nmap,
                           const float *g_entropy, const float *g_weights, float *g_sdf, float *g_rgb, float *g_grad,
                           nsa_stream_t stream);

/* x = o + z d, view dir = d:  d/d(rays_o)[R,3] = sum_i g_x ;  d/d(rays_d)[R,3] = sum_i z_i g_x + sum_i g_dir. */
int nsa_rays_backward(const float *z_vals, const float *g_x, const float *g_dir, uint32_t R, uint32_t S,
                      float *g_rays_o, float *g_rays_d, nsa_stream_t stream);

/* Coarse sampler stage: stratified z on [near, cube exit], points, coarse+fine SDF at R*E points (no grad).
 * replaces UniformSampler.get_z_vals (code/model/ray_sampler.py:37-61) + ImplicitNetworkGrid_COMBINE.get_sdf_vals
 * (code/model/base_networks.py:27-32) as called from ImportantSampler.get_z_vals (ray_sampler.py:92-102).
 * t_lin = linspace(0,1,E); t_rand = per-sample jitter in [0,1) or NULL (eval mode); packed_* = MLP parameters
 * in MFMA fragment order (nicer_slam_amd/fused/pack.py).  Outputs z[R,E], sdf[R,E], far[R]. */
int nsa_sampler_sdf(const float *rays_o, const float *rays_d, uint32_t R, uint32_t E, const float *t_lin,
                    const float *t_rand, float near, float bound, float far_cap, const nsa_grid_t *coarse,
                    const nsa_grid_t *fine, const float *packed_coarse, const float *packed_fine, float *z,
                    float *sdf, float *far, nsa_stream_t stream);

/* Per-ray importance stage: density -> weights -> cdf -> N inverse-CDF samples, merged with near, far and
 * n_extra of the coarse samples, sorted.  replaces ImportantSampler.get_z_vals (ray_sampler.py:104-159) and
 * GridPredefineDensity (code/model/density.py:37-67).  z_vals[R, N+2+n_extra]; z_eik[R] = z_vals[r, eik_idx[r]]
 * (optional).  One workgroup per ray; N+2+n_extra <= 256, voxel_res <= 1024. */
int nsa_sample_rays(const float *rays_o, const float *rays_d, const float *z, const float *sdf, const float *far,
                    const float *voxels, uint32_t voxel_res, uint32_t R, uint32_t E, uint32_t N, const float *u_lin,
                    const int32_t *extra_idx, uint32_t n_extra, float near, const int32_t *eik_idx, float *z_vals,
                    float *z_eik, nsa_stream_t stream);

/* ---- Section 3: scalar head/tail of a tracking iteration (so a whole iteration is a fixed kernel sequence) ---- */

/* cam[b,7] = (qw,qx,qy,qz,tx,ty,tz) -> pose[b,4,4].  replaces quad2rotation / get_camera_from_tensor
 * (code/utils/general.py:52-100); nsa_pose_grad_to_cam is its backward (g_pose[b,4,4] -> g_cam[b,7]). */
int nsa_cam_to_pose(const float *cam, uint32_t b, float *pose, nsa_stream_t stream);
int nsa_pose_grad_to_cam(const float *cam, const float *g_pose, uint32_t b, float *g_cam, nsa_stream_t stream);

/* loss[0] = mean |pred - target| over n scalars, g_pred = sign(pred - target)/n.  replaces SLAMLoss.get_rgb_loss with
 * torch.nn.L1Loss(reduction="mean") (code/model/loss.py:57-65,131) and its backward. */
int nsa_l1_loss(const float *pred, const float *target, uint32_t n, float *loss, float *g_pred, nsa_stream_t stream);

/* torch.optim.Adam step (no weight decay / amsgrad) on n <= 256 parameters; `step` is a device scalar that is
 * incremented; lr_step > 0 applies StepLR(lr_step, lr_gamma).  replaces optimizer_camera.step() +
 * scheduler_camera.step() (code/training/volsdf_train.py:396-399,425-427). */
int nsa_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, uint32_t n,
                  float lr, float beta1, float beta2, float eps, uint32_t lr_step, float lr_gamma,
                  nsa_stream_t stream);

/* Integer draws of one sampler call from a buffer u of E + R uniforms in [0,1): extra_idx[n_extra] = the first n_extra
 * entries of a random permutation of 0..E-1 (E <= 1024), eik_idx[R] = uniform in 0..S-1; either output may be NULL.
 * replaces torch.randperm(E)[:n_extra] and torch.randint(S, (R,)) (code/model/ray_sampler.py:148,158). */
int nsa_draw_picks(const float *u, uint32_t E, uint32_t n_extra, uint32_t R, uint32_t S, int32_t *extra_idx,
                   int32_t *eik_idx, nsa_stream_t stream);

/* Every random draw of one sampler call in one launch, from a counter-based generator (Philox4x32-10, the generator behind
 * torch.rand) whose state the caller owns: state = 4 x uint64 on the device {seed, call number, 0, 0}; the kernel advances the
 * call number itself, so a captured graph draws fresh numbers on every replay.  t_rand[n_rand] uniforms in [0,1) (the stratified
 * jitter, ray_sampler.py:57-58), extra_idx / eik_idx as nsa_draw_picks (any output may be NULL).  Value i of call c is
 * philox(key = seed, counter = (i / 4, region, c))[i % 4] >> 8, region 0 = t_rand, 1 = the E permutation keys, 2 = eik_idx.
 * replaces torch.rand / torch.randperm / torch.randint of code/model/ray_sampler.py:57-58,148,158. */
int nsa_draw(uint64_t *state, uint64_t n_rand, float *t_rand, uint32_t E, uint32_t n_extra, uint32_t R, uint32_t S,
             int32_t *extra_idx, int32_t *eik_idx, nsa_stream_t stream);

/* SDF (coarse + fine; fine == NULL: stage "coarse") at N explicit points, no gradients: batch inference for mesh
 * extraction grids and plots.  replaces ImplicitNetworkGrid_COMBINE.get_sdf_vals (code/model/base_networks.py:25-35)
 * as called by code/utils/plots.py:91,142. */
int nsa_sdf_points(const float *points, uint64_t N, const nsa_grid_t *coarse, const nsa_grid_t *fine,
                   const float *packed_coarse, const float *packed_fine, float *sdf, nsa_stream_t stream);

/* Fused head and tail of a single-image tracking iteration (graph-captured tracker): fewer, larger graph nodes.
 *   nsa_track_head = nsa_cam_to_pose + nsa_rays_forward (b = 1);
 *   nsa_track_tail = nsa_rays_pose_backward + nsa_pose_grad_to_cam (g_cam[7]) and, with do_adam != 0, nsa_adam_step on the
 *   camera vector -- the same arithmetic in one block.  Reference: the lines those four entry points cite. */
int nsa_track_head(const float *uv, const float *K, const float *cam, uint32_t n, float *pose, float *rays_o,
                   float *rays_d, float *depth_scale, nsa_stream_t stream);
int nsa_track_tail(const float *uv, const float *K, float *cam, uint32_t n, const float *g_rays_o, const float *g_rays_d,
                   float *g_cam, int do_adam, float reduce_weight, float *exp_avg, float *exp_avg_sq, float *step, float lr,
                   float beta1, float beta2, float eps, uint32_t lr_step, float lr_gamma, const float *loss, float *best,
                   nsa_stream_t stream);
/* `best` (optional, 8 floats, with do_adam): the arg-min-loss camera of the frame -- best[0] = smallest loss[0] seen,
 * best[1..7] = the camera AFTER the step of that iteration (strict <).  replaces candidate_cam_tensor / current_min_loss
 * (code/training/volsdf_train.py:402-403,441-446).  Start a frame with best[0] = 1e10. */
/* Multi-GPU form: reduce_weight = this rank's ray count > 0 turns g_cam into the 9-float message
 * [w*g_cam(7), w*loss (slot 7 as left by nsa_l1_loss), w] that is summed over ranks with ONE all-reduce; the step is then
 * nsa_adam_step_scaled(cam, msg, msg + 8, ...) = Adam on msg[0..6] / msg[8]. */
/* The same iteration with the per-ray neighbours folded in (one ray chunk; what the graph-captured tracker runs):
 *   nsa_track_begin     = copy of the frame's pixel batch (uv_in [n,2], gt_in [n,3]) into the resident buffers uv / gt that the
 *                         captured sequence reads + nsa_track_head -- one launch in front of the graph replay;
 *   nsa_composite_track = nsa_composite_forward (rendered colour only) + nsa_l1_loss + nsa_composite_backward(g_rgb_values) in
 *                         one pass per ray; ray_loss[r] = sum_c |rgb_values[r,c] - gt[r,c]|, the cotangent is sign / (3 n_total);
 *                         g_grad is zero-filled (the tracking objective has no normal-map term)
 *                         (code/model/network.py:349-370, loss.py:57-65,131);
 *   nsa_track_finish    = nsa_rays_backward + nsa_track_tail, the loss (slot 7 of g_cam) formed as sum(ray_loss) / (3 n) from
 *                         fixed-order block partials by the last block to arrive: deterministic.  `workspace`:
 *                         nsa_track_finish_workspace(n) floats, zero-filled ONCE by the caller (the kernel leaves its ticket zero).
 *                         `best` compares g_cam[7]. */
int nsa_track_begin(const float *uv_in, const float *gt_in, float *uv, float *gt, const float *K, const float *cam, uint32_t n,
                    float *pose, float *rays_o, float *rays_d, float *depth_scale, nsa_stream_t stream);
/* nsa_track_begin and the iteration's sampler draws (nsa_draw with n_rand uniforms into t_rand, the n_extra picks of E into
 * extra_idx, no eikonal picks; R = n) in ONE launch: the draw's workgroups ride beside the ray lifting instead of being a graph
 * node of their own.  Same draws, bit for bit, as nsa_draw on the same state. */
int nsa_track_begin_draw(const float *uv_in, const float *gt_in, float *uv, float *gt, const float *K, const float *cam, uint32_t n,
                         float *pose, float *rays_o, float *rays_d, float *depth_scale, uint64_t *state, uint64_t n_rand,
                         float *t_rand, uint32_t E, uint32_t n_extra, uint32_t S, int32_t *extra_idx, nsa_stream_t stream);
int nsa_composite_track(const float *rays_o, const float *rays_d, const float *z_vals, const float *sdf, const float *rgb,
                        const float *voxels, uint32_t voxel_res, uint32_t R, uint32_t S, const float *gt, uint32_t n_total,
                        float *rgb_values, float *ray_loss, float *g_sdf, float *g_rgb, float *g_grad, nsa_stream_t stream);
int nsa_track_finish(const float *uv, const float *K, float *cam, uint32_t n, uint32_t S, const float *z_vals, const float *g_x,
                     const float *g_dir, const float *ray_loss, float *g_cam, int do_adam, float reduce_weight, float *exp_avg,
                     float *exp_avg_sq, float *step, float lr, float beta1, float beta2, float eps, uint32_t lr_step,
                     float lr_gamma, float *best, float *workspace, nsa_stream_t stream);
uint64_t nsa_track_finish_workspace(uint32_t n);
int nsa_adam_step_scaled(float *param, const float *grad, const float *grad_div, float *exp_avg, float *exp_avg_sq,
                         float *step, uint32_t n, float lr, float beta1, float beta2, float eps, uint32_t lr_step,
                         float lr_gamma, const float *loss, float *best, nsa_stream_t stream);
/* (loss, best: as for nsa_track_tail, best[1..n]; the loss compared is loss[0] / grad_div[0]) */

/* ---- Section 4: mapping-iteration tail ------------------------------------------------------------------------ */

/* keys[i] = 30-bit Morton code of point i in a 1024^3 lattice over [-1,1]^3; argsort(keys) is a spatially coherent
 * launch order for nsa_points_t.order (new -- the reference processes points in ray order). */
int nsa_morton_keys(const nsa_points_t *pts, int32_t *keys, nsa_stream_t stream);

/* order[] = stable argsort of the top `key_bits` (1..30) bits of those keys: the launch order itself, by an in-library LSD radix
 * sort (8-bit digits, two launches per pass, deterministic).  workspace: nsa_morton_order_workspace(P) 4-byte words.
 * (new, as nsa_morton_keys; replaces keys -> torch.sort -> indices.) */
int nsa_morton_order(const nsa_points_t *pts, int32_t *order, uint32_t *workspace, uint32_t key_bits, nsa_stream_t stream);
uint64_t nsa_morton_order_workspace(uint32_t P);

/* voxels[floor((x+1)/2*res)] += 1 for every sample with all |x_d| <= 0.99 (voxels: [res,res,res] fp32, x-major).
 * replaces SLAMNetwork.update_voxels (code/model/network.py:62-76). */
int nsa_update_voxels(const nsa_points_t *pts, float *voxels, uint32_t res, nsa_stream_t stream);

/* One torch.optim.Adam step (no weight decay / amsgrad) over n parameters in a single pass; `step` = this step's
 * number t >= 1 (bias corrections are computed on the host in double, like torch).  16-byte aligned pointers take the
 * 16-byte path; anything less (4-byte aligned at least) a one-element-per-thread form with the same arithmetic.
 * replaces self.optimizer.step() for one parameter tensor (code/training/volsdf_train.py:174, 420-424). */
int nsa_adam_table_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, uint64_t n, uint32_t step,
                        float lr, float beta1, float beta2, float eps, nsa_stream_t stream);

/* The same step with the gradient CONSUMED: every gradient element read is left zero (16-byte groups that were already zero are
 * not rewritten), so a persistent gradient buffer needs no zero fill before the next backward pass scatters into it.
 * replaces optimizer.step() + the next iteration's optimizer.zero_grad() / dense zero-initialised table gradient
 * (code/training/volsdf_train.py:547-576, code/hashencoder/hashgrid.py:117-118) for one table. */
int nsa_adam_table_step_clear(float *param, float *grad, float *exp_avg, float *exp_avg_sq, uint64_t n, uint32_t step,
                              float lr, float beta1, float beta2, float eps, nsa_stream_t stream);

/* The step of a parameter that received NO gradient this iteration, as the reference's environment takes it: under torch 1.11
 * (env_yamls/nicer-slam.yaml:62) optimizer.zero_grad() (code/training/volsdf_train.py:547) leaves zero TENSORS, so Adam still decays both
 * moments and moves the parameter along its momentum (the fine table during stage "coarse", the colour table during color_stage "base",
 * :550-555); torch >= 2.0 sets .grad = None and skips such a parameter.  Arithmetic of nsa_adam_table_step with grad == 0, no gradient
 * read (3 reads + 3 writes per element).  replaces zero_grad() + optimizer.step() for one un-touched tensor (volsdf_train.py:547,576). */
int nsa_adam_table_step_zero_grad(float *param, float *exp_avg, float *exp_avg_sq, uint64_t n, uint32_t step, float lr, float beta1,
                                  float beta2, float eps, nsa_stream_t stream);

/* The same Adam step over up to 24 SMALL tensors (n <= 2^24 each) in one launch: the weight_v / weight_g / bias tensors of the
 * trained MLPs.  Per-tensor lr and step count; beta1, beta2, eps shared.  4-byte aligned pointers suffice. */
typedef struct nsa_adam_seg {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    uint32_t n, step;
    float lr;
} nsa_adam_seg_t;
int nsa_adam_multi_step(const nsa_adam_seg_t *segs, uint32_t count, float beta1, float beta2, float eps, nsa_stream_t stream);

/* p[0..n) = 0 (p 16-byte aligned): the zero fill of a table-gradient buffer as a library launch, issued on the launch stream right
 * before the first backward kernel of a pass scatters into the buffer (nicer_slam_amd/fused/tablegrad.py).  replaces optimizer.zero_grad() +
 * the zero-initialised dense gradient of code/hashencoder/hashgrid.py:117-118. */
int nsa_fill_zero(float *p, uint64_t n, nsa_stream_t stream);

/* Weight-normed Linear layers -> the flat effective parameter vector the packed blocks and the MAP kernels' gradients use:
 *   flat = [W_0 (rows x cols, row-major), b_0, W_1, b_1, .., 0],   W_l[r,:] = weight_v_l[r,:] * weight_g_l[r] / ||weight_v_l[r,:]||,
 * norms[row] = ||weight_v_l[r,:]|| for the backward (rows of all layers, in order); n_layers <= 8.
 * replaces nn.utils.weight_norm's per-layer recomputation (torch._weight_norm, dim 0) of code/model/base_networks.py:137-141,
 * 376-379 + the reshape / cat that followed it here. */
typedef struct nsa_wn_layer {
    const float *weight_v;   /* [rows, cols] */
    const float *weight_g;   /* [rows]       */
    const float *bias;       /* [rows]       */
    uint32_t rows, cols;
} nsa_wn_layer_t;
int nsa_weight_norm_flat(const nsa_wn_layer_t *layers, uint32_t n_layers, float *flat, float *norms, nsa_stream_t stream);
/* Its backward: g_flat (layout of flat) -> g_params = per layer [g_weight_v (rows x cols) | g_weight_g (rows) | g_bias (rows)]. */
int nsa_weight_norm_flat_backward(const nsa_wn_layer_t *layers, uint32_t n_layers, const float *norms, const float *g_flat,
                                  float *g_params, nsa_stream_t stream);

/* One extra emission row for nsa_emit_gemm: dst[p] = src[order ? order[p] : p] (src NULL: `fill`) for p < P, 0 for P <= p < n. */
int nsa_emit_row(float *dst, const float *src, const int32_t *order, uint32_t P, uint64_t n, float fill, nsa_stream_t stream);

/* Packed MLP parameter block (MFMA fragment order) from the flat effective parameters in one launch:
 *   out[o] = word order[o] of concat( split(flat[a_index]) as [group][piece 0/1/2][lane][4 words of 2 halfwords], flat[v_index] )
 * (the pieces: nsa_operand_form)
 * a_index: n_a = groups * 64 * 8 indices into `flat` (the 8 fp32 weights lane l supplies to one MFMA k-group; every weight is
 * split exactly into three round-to-nearest bf16 pieces), v_index: n_v indices of per-feature values kept in fp32, order:
 * n_out <= n_a * 3 / 2 + n_v word indices into that concatenation.  The index arrays are the host-built layout tables of the
 * packed blocks (nicer_slam_amd/fused/pack.py; layout: csrc/mlp_common.hpp, csrc/mlp16.hpp).  New -- the reference has no
 * packed weights; replaces the per-layer weight_norm'ed nn.Linear weights of code/model/base_networks.py:127-149 as kernel input. */
/* How this library's fp32 path feeds the matrix cores, i.e. what nsa_pack_blocks writes into a fragment triple: 3 = three exact bf16
 * pieces of the weight (hi / mid / lo), 2 = two fp16 pieces of 512 w (round-to-nearest twice) + the bf16 round-to-nearest value for
 * the bf16-operand kernels.  A build-time choice (csrc/mlp_common.hpp::NSA_FORM); host code that builds packs itself (the
 * differentiable fallback of fused/pack.py) asks.  New -- no reference counterpart. */
int nsa_operand_form(void);

int nsa_pack_blocks(const float *flat, const int64_t *a_index, uint64_t n_a, const int64_t *v_index, uint64_t n_v,
                    const int64_t *order, uint64_t n_out, float *out, nsa_stream_t stream);

/* MLP weight gradients from the emission rows of the *_backward_params kernels: emit is [rows][ld] fp32 (column = point,
 * ld a multiple of 4096, columns past the last point zero).
 *   out[m][n] = sum_j sum_p emit[a_rows[j] + m][p] * emit[b_rows[j] + n][p],   j < pairs (1 or 2), m < M <= 64, n < N <= 192
 * and, with row_sums, out[m][N] = sum_p emit[a_rows[0] + m][p] (the bias gradient); out is [M][N + row_sums], fp32-faithful
 * products, deterministic (per-chunk partials in `workspace`, nsa_emit_gemm_workspace() floats, added in chunk order).
 * replaces torch autograd's weight / bias gradients of the Linear layers (code/model/base_networks.py:195-221, 333-395). */
int nsa_emit_gemm(const float *emit, uint64_t ld, uint32_t pairs, const uint32_t *a_rows, const uint32_t *b_rows, uint32_t M,
                  uint32_t N, int row_sums, float *out, float *workspace, nsa_stream_t stream);
uint64_t nsa_emit_gemm_workspace(uint64_t ld, uint32_t M, uint32_t N, int row_sums);

/* The per-ray terms of SLAMLoss (code/model/loss.py:113-233: rgb L1, eikonal, smooth, scale-and-shift-invariant monocular
 * depth with its alpha = 0.5 first-difference regulariser (code/utils/MiDaS.py:6-143), gt-depth L1, normal L1 + cos) and the
 * gradient of their WEIGHTED sum w.r.t. the model outputs, in three launches.  A weight of 0 skips a term (its value is then 0,
 * like the reference's 0.0); the flow and patch-warp terms are Section 5.  R = bs * n rays, image-major. */
typedef struct nsa_loss {
    uint32_t bs, n;               /* images, rays per image                                                             */
    uint32_t S;                   /* samples per ray of `sdf`                                                           */
    uint32_t E;                   /* eikonal points (0: no eikonal / smooth term)                                       */
    const float *rgb, *rgb_gt;    /* [R,3] rgb_values, ground_truth['rgb']                                              */
    const float *depth;           /* [R]   depth_values                                                                 */
    const float *depth_mono;      /* [R]   ground_truth['depth'] (monocular; the term aligns to 50 * it + 0.5)           */
    const float *depth_real;      /* [R]   target of the gt-depth L1 term (gt_depth, or depth * assign_scale on frame 0) */
    const float *depth_real_mask; /* [R]   the gt-depth term covers rays with this > 0 (ground_truth['gt_depth'])        */
    const float *mask_gt;         /* [R]   ground_truth['mask'] (foreground where > 0.5 AND the ray's sdf changes sign)  */
    const float *sdf;             /* [R,S] */
    const float *normal, *normal_gt;             /* [R,3] normal_map, ground_truth['normal']                            */
    const float *grad_theta, *grad_theta_nei;    /* [E,3]; grad_theta_nei may be NULL (no smooth term)                  */
    float w_rgb, w_eik, w_smooth, w_depth, w_gtdepth, w_nl1, w_ncos;
    int depth_whole_image;        /* depth term over every ray instead of the foreground (Replica scan 4, loss.py:171-175) */
    float *g_rgb, *g_depth, *g_normal, *g_theta, *g_theta_nei;   /* out: d(weighted sum) / d(input), same shapes         */
    float *terms;                 /* out [8]: rgb, eikonal, smooth, depth, gt_depth, normal_l1, normal_cos (unweighted), sum */
} nsa_loss_t;
int nsa_slam_loss(const nsa_loss_t *in, float *workspace /* nsa_slam_loss_workspace() floats, 8-byte aligned */,
                  nsa_stream_t stream);
uint64_t nsa_slam_loss_workspace(uint32_t bs, uint32_t n, uint32_t E);

/* ---- Section 5: keyframe re-projection blocks of a mapping iteration (patch warp, flow), their masked-L1 and patch-SSIM terms ---- */

/* Shared description of a mapping batch: b keyframes x n sampled pixels.  `images` / `depths` are the resident full frames
 * ([frames,H,W,3] / [frames,H,W] fp32, pixel (y,x) at y*W+x -- the reference's ground_truth['full_rgb'] / ['full_depth'],
 * code/datasets/scene_dataset.py:248-257); batch entry i uses frame frame_index[i] of that store (NULL: frame i), so a
 * batch needs no per-iteration stacking copy of the frames. */
typedef struct nsa_warp {
    uint32_t b, n;              /* keyframes in the batch, sampled pixels per keyframe                                  */
    uint32_t H, W;              /* image size                                                                           */
    const float *uv;            /* [b,n,2] pixel coordinates                                                            */
    const float *pose;          /* [b,4,4] camera-to-world                                                              */
    const float *w2c;           /* [b,4,4] its inverse (the caller forms it with torch.linalg.inv like network.py:157,191) */
    const float *K;             /* [b,4,4] intrinsics                                                                   */
    const float *depth;         /* [b,n]   rendered depth along the ray, BEFORE the depth_scale factor (network.py:147-150) */
    const float *images;        /* [frames,H,W,3]                                                                       */
    const float *depths;        /* [frames,H,W]   (patch > 1 only; may be NULL otherwise)                               */
    const int32_t *frame_index; /* [b] device, or NULL                                                                  */
} nsa_warp_t;

/* Patch warp, forward: for every (target t, source s, pixel i, patch cell c) the reference's warp_output[patch] tensors
 *   sampled[t,s,i,c,3] = bilinear sample (zeros padding, align_corners=True) of image t at the projection of the lifted cell,
 *   gt_rgb [t,s,i,c,3] = image s at the cell's own pixel (ones outside the image), replicated over t,
 *   mask   [t,s,i,c]   = projection strictly inside image t and in front of it  &  cell inside image s  &  (patch > 1) flat[s,i],
 *   flat   [s,i]       = biased variance of the patch's ground-truth depths < 0.01 (patch > 1; else untouched, may be NULL).
 * Cell order c = ix * patch + iy with offsets (ix - patch/2, iy - patch/2) on (u,v) (general.py:139-144); patch must be odd.
 * replaces code/model/network.py:167-279 (one patch size per call) + uv2patch (code/utils/general.py:129-145). */
int nsa_patch_warp_forward(const nsa_warp_t *in, uint32_t patch, float *sampled, uint8_t *mask, float *gt_rgb, uint8_t *flat,
                           nsa_stream_t stream);

/* Backward of the above: g_sampled[t,s,i,c,3] -> g_depth[b,n] (overwritten); when g_pose and g_w2c are non-NULL also the
 * gradients of the source poses (through ray origin and direction) and of the target world-to-camera matrices, both [b,4,4]
 * (overwritten, bottom row zero) -- bundle adjustment (volsdf_train.py:521-528).  Deterministic (fixed-order sums).
 * workspace: nsa_patch_warp_workspace() floats (may be NULL when that is 0). */
int nsa_patch_warp_backward(const nsa_warp_t *in, uint32_t patch, const float *g_sampled, float *g_depth, float *g_pose,
                            float *g_w2c, float *workspace, nsa_stream_t stream);
uint64_t nsa_patch_warp_workspace(uint32_t b, uint32_t n, uint32_t patch, int want_pose);

/* Flow: flow[e,i,2] = projection into frame idjj[e] of the rendered point of pixel i of frame idii[e], minus that pixel.
 * idii / idjj: [ne] int64 on the device (the reference's `edges`, volsdf_train.py:312-324).  replaces network.py:153-165.
 * (`images`, `depths` of nsa_warp_t are not used.) */
int nsa_flow_forward(const nsa_warp_t *in, const int64_t *idii, const int64_t *idjj, uint32_t ne, float *flow,
                     nsa_stream_t stream);
int nsa_flow_backward(const nsa_warp_t *in, const int64_t *idii, const int64_t *idjj, uint32_t ne, const float *g_flow,
                      float *g_depth, float *g_pose, float *g_w2c, float *workspace, nsa_stream_t stream);
uint64_t nsa_flow_workspace(uint32_t b, uint32_t n, uint32_t ne, int want_pose);

/* loss[0] = mean over the selected items and their `channels` values of |pred - target| (NaN for an empty selection, like
 * torch); g_pred (optional, [items,channels]) = its gradient, 0 outside the mask.  mask: [items] bytes or NULL (all).
 * replaces `(sampled[mask] - gt[mask]).abs().mean()` (code/model/loss.py:136-142) and the flow L1 on flow_mask (:106-111).
 * workspace: nsa_masked_l1_workspace() floats, 8-byte aligned.  Deterministic. */
int nsa_masked_l1(const float *pred, const float *target, const uint8_t *mask, uint64_t items, uint32_t channels, float *loss,
                  float *g_pred, float *workspace, nsa_stream_t stream);
uint64_t nsa_masked_l1_workspace(uint64_t items);

/* The SSIM form of the patch-warp term (warp_loss_type = "ssim", code/model/loss.py:51-55,145-152: pytorch_msssim's SSIM with
 * data_range 1 and a sigma-1.5 Gaussian window as large as the patch, so one value per patch and channel).  pred, target:
 * [n_patches, patch^2, 3] fp32; mask: [n_patches, patch^2] bytes or NULL (all); both images count as 0 where the mask is
 * false (zeroed, not excluded).  Per patch and channel, in float64 with w_ij = g_i * g_j the exact product of the fp32 window:
 *   mu_x = sum w x, mu_y = sum w y, s_xx = sum w x^2 - mu_x^2, s_yy = sum w y^2 - mu_y^2, s_xy = sum w x y - mu_x mu_y
 *   SSIM = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * (2 s_xy + C2) / (s_xx + s_yy + C2),   C1 = 1e-4, C2 = 9e-4
 * loss[0] = 1 - mean of the 3 * n_patches values, rounded once to fp32 (the reference's term is 0.05 * loss[0]); a wholly masked
 * patch counts with SSIM exactly 1; pred == target gives exactly 0; n_patches == 0 gives NaN (torch's mean of nothing) and is not
 * an error.  g_pred (optional, pred's layout) = d loss[0] / d pred, rounded once, exactly 0 where the mask is false.
 * patch: odd, 3 .. 11, and 3 * patch^2 * n_patches < 2^31.  workspace: nsa_patch_ssim_workspace() floats, 8-byte aligned.
 * Two launches, no atomics: bit-identical from run to run, and a patch's gradient does not depend on its place in the batch. */
int nsa_patch_ssim(const float *pred, const float *target, const uint8_t *mask, uint64_t n_patches, uint32_t patch, float *loss,
                   float *g_pred, float *workspace, nsa_stream_t stream);
uint64_t nsa_patch_ssim_workspace(uint64_t n_patches);

/* ---- Section 6: per-iteration input batch from frames resident in HBM ------------------------------------------------ */

/* One field of the frame stores: store [capacity, pixels, channels] fp32, out [b, n, channels]. */
typedef struct nsa_feed_field {
    const float *store;
    float *out;
    uint32_t channels; /* 1..16 */
} nsa_feed_field_t;

/* out_f[i,k,:] = store_f[slots[i], sel[k], :] for every field (at most 8), uv[i,k] = (sel[k] % width, sel[k] / width) (uv may be
 * NULL) in one launch.  slots: [b] int32 store slots of the batch's frames, sel: [n] int64 pixel indices (an index outside
 * [0, pixels) yields NaN rows).  replaces SLAMDataset.__getitem__'s `[self.sampling_idx, :]` of every image + collate_fn
 * (code/datasets/scene_dataset.py:214-275) for frames kept on the device (nicer_slam_amd/feed.py). */
int nsa_feed_gather(const nsa_feed_field_t *fields, uint32_t n_fields, const int32_t *slots, uint32_t b, const int64_t *sel,
                    uint32_t n, uint64_t pixels, uint32_t width, float *uv, nsa_stream_t stream);

/* Up to 8 float segments (dst[i][0..n) = src[i][0..n), device pointers) copied in ONE launch: the per-call inputs of a cached graph
 * (pose, pixel batch, intrinsics -- the `.cuda()` / copy of each model input in the reference's loop, volsdf_train.py:411-416). */
typedef struct nsa_copy_seg {
    float *dst;
    const float *src;
    uint32_t n; /* floats */
} nsa_copy_seg_t;
int nsa_copy_segments(const nsa_copy_seg_t *segs, uint32_t n_segs, nsa_stream_t stream);

/* ---- Section 7: mesh extraction (marching cubes over a dense fp32 volume; DESIGN 4f, csrc/mesh_extract.hip) ------------- */

/* vol[nx, ny, nz] C-contiguous, sample (x, y, z) at (x * ny + y) * nz + z -- the layout nicer_slam_amd.inference.sdf_grid returns.
 * Inside is value < level.  One vertex per grid edge whose two samples are finite and on opposite sides, at
 *   t = (level - f0) / (f1 - f0),  p_k = origin_k + spacing_k * c_k,  c_k = (float)i_k (k != axis a), c_a = (float)i_a + t
 * (fp32, no FMA contraction; f0 at the edge's lower sample i).  Its normal is the central-difference volume gradient
 * (one-sided on the border) interpolated with t and normalised, pointing towards increasing value (0 when the interpolated
 * gradient is zero or not finite).  A cell with a non-finite corner emits no faces.  Vertices are ordered by (lower sample,
 * axis), faces [F,3] int32 by (cell, case-table order; csrc/mc_table.hpp), oriented inside -> outside.  nx * ny * nz <= 2^31;
 * a dimension below 2 gives an empty mesh.  Nothing is allocated or synchronised; the workspace belongs to the caller.
 * Together these replace skimage.measure.marching_cubes (code/utils/plots.py:128, spacing :130-134, origin :136). */

/* bytes of workspace for a volume of nx * ny * nz samples */
uint64_t nsa_marching_cubes_workspace(uint32_t nx, uint32_t ny, uint32_t nz);

/* Phase 1: classify every cell and edge and write totals[2] = {vertices, faces} (uint64, device) for nsa_marching_cubes_emit. */
int nsa_marching_cubes_count(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, void *workspace,
                             uint64_t *totals, nsa_stream_t stream);

/* Phase 2, after phase 1 on the same volume, level and workspace: verts[n_verts, 3], normals[n_verts, 3], faces[n_faces, 3]
 * with n_verts, n_faces the totals of phase 1 (read by the caller to size the outputs; nothing past them is written).
 * origin_host[3] / spacing_host[3] per axis (spacing finite and > 0).  A total above INT32_MAX returns NSA_EMESH_TOO_LARGE. */
int nsa_marching_cubes_emit(const float *vol, uint32_t nx, uint32_t ny, uint32_t nz, float level, const float *origin_host,
                            const float *spacing_host, void *workspace, uint64_t n_verts, uint64_t n_faces, float *verts,
                            float *normals, int32_t *faces, nsa_stream_t stream);

/* ---- Section 8: mesh evaluation (exact nearest neighbours, surface sampling; DESIGN 4g, csrc/mesh_eval.hip) -------------- */

/* Exact nearest neighbour, point cloud to point cloud.  targets[n_targets, 3] and queries[n_queries, 3] fp32, C-contiguous.
 * For query q the answer is the target i with the smallest fp32
 *     d2 = (dx * dx + dy * dy) + dz * dz,   dk = t_ik - q_k,   every operation rounded on its own (no FMA contraction),
 * ties to the LOWEST index; dist = the correctly rounded fp32 square root of d2 (IEEE sqrtf).  Any fp32 brute force with this operation order reproduces
 * (idx, dist) bit for bit.  A target with a non-finite coordinate is never returned; a non-finite query gives (-1, NaN).
 * Radius: with max_dist < +inf a target is accepted only if d2 < (float)(max_dist * max_dist) -- strictly, as the radius search
 * of open3d's KDTreeFlann::SearchHybrid inside registration_icp (eval_rec.py:197-203); a query with no accepted target gives
 * (-1, +inf).  max_dist = +inf is the plain search (scipy cKDTree.query, eval_rec.py:18, :111, :172-186).
 * The index is a uniform grid over the bulk of the targets with per-cell bounding boxes; it is built once and
 * reused by every query on it.  Counts are below 2^31.  Nothing is allocated or synchronised; the index buffer belongs to the
 * caller and must stay alive, and the targets unchanged, only while nsa_nn_build runs (the index holds its own copy). */

/* bytes of the index buffer for n_targets (>= 1) targets; 0 for an invalid count */
uint64_t nsa_nn_workspace(uint32_t n_targets);

/* Build the index over targets into `index` (nsa_nn_workspace(n_targets) bytes, device, 256-byte aligned). */
int nsa_nn_build(const float *targets, uint32_t n_targets, void *index, nsa_stream_t stream);

/* idx[n_queries] int32, dist[n_queries] fp32 for queries against an index built by nsa_nn_build with the same n_targets.
 * max_dist > 0 (+inf: no radius). */
int nsa_nn_query(const void *index, uint32_t n_targets, const float *queries, uint32_t n_queries, double max_dist, int32_t *idx,
                 float *dist, nsa_stream_t stream);

/* Area-weighted surface sampling: restates trimesh.sample.sample_surface (eval_rec.py:158, :222, :225).  verts[n_verts, 3] fp32,
 * faces[n_faces, 3] int32 (a face with an index outside [0, n_verts) has area 0).  Areas a_f = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz),
 * c = (v1 - v0) x (v2 - v0) in float64; cum[f] = boff[b] + local[f] with local the sequential inclusive scan within blocks of
 * 1024 faces and boff the sequential sum of the earlier block totals, so cum is non-decreasing; total = cum[F - 1].
 * Sample s draws Philox4x32-10 with key = seed, counter = (s, 0, 0, 0) -> (c0, c1, c2, c3):
 *   face_idx[s] = first f with cum[f] >= ((c0 >> 8) + 1) * 2^-24 * total   (u in (0, 1]: zero-area faces are never picked)
 *   a = (c1 >> 8) * 2^-24, b = (c2 >> 8) * 2^-24 (fp32); when a + b > 1 (fp32): a = 1 - a, b = 1 - b
 *   points[s] = (v0 + a * (v1 - v0)) + b * (v2 - v0), fp32, each operation rounded on its own.
 * total_area (device, may be NULL) receives the total; when it is 0 or not finite the samples are meaningless and the caller
 * rejects the mesh.  Nothing is allocated or synchronised; the workspace belongs to the caller. */

/* bytes of workspace for n_faces (>= 1) faces; 0 for an invalid count */
uint64_t nsa_surface_sample_workspace(uint32_t n_faces);

int nsa_surface_sample(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, uint32_t n_samples,
                       uint64_t seed, void *workspace, float *points, int32_t *face_idx, double *total_area, nsa_stream_t stream);

/* ---- Section 9: rendering metrics (PSNR and SSIM of image pairs in float64; DESIGN 4h, csrc/image_metrics.hip) ------------ */

/* pred[n_images, height * width, 3] and gt[same] fp32, C-contiguous, pixel (r, c) at r * width + c -- the layout of rgb_values
 * and ground_truth["rgb"].  Per image, the SSIM of code/utils/SSIM with size_average=True (as rend_util.get_ssim calls it) and
 * the sum of squared errors of rend_util.get_psnr, every value converted to float64 before any arithmetic:
 *   window   g_k = (float)exp(-(k - 5)^2 / 4.5), k = 0..10, each divided (fp32) by their correctly rounded fp32 sum;
 *            w_ij = g_i * g_j EXACTLY (float64; the reference rounds it to fp32, which moves SSIM by < 4e-7)
 *   moments  per channel, zero padding of 5 on every side: mu_x = sum w x, mu_y = sum w y, e_xx = sum w x^2,
 *            e_yy = sum w y^2, e_xy = sum w x y (float64)
 *   map      ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),  C1 = 1e-4, C2 = 9e-4,
 *            s_xx = e_xx - mu_x^2, s_yy = e_yy - mu_y^2, s_xy = e_xy - mu_x mu_y, each operation rounded on its own
 *   ssim_mean[i]  = (sum of the map over the 3 channels and height * width pixels) / (3 * height * width)   (float64)
 *   sq_err_sum[i] = sum over the 3 * height * width values of (x - y)^2   (float64; PSNR = -10 log10(sq_err_sum / count))
 *   ssim_map[i, r, c] (optional, fp32 [n_images, height, width]) = the float64 mean of the three channels' map values, rounded.
 * An image scored against itself gives ssim_mean = 1 and sq_err_sum = 0 exactly.  Any non-finite value in either image of a pair
 * makes both of its outputs NaN (the map is NaN within 5 pixels of it).  The sums are taken in a fixed order: results are
 * bit-reproducible and do not depend on the other images of the batch.  n_images * height * width * 3 < 2^31.  Nothing is
 * allocated or synchronised; the workspace belongs to the caller.  Together these replace rend_util.get_psnr / get_ssim
 * (code/evaluation/eval_rendering.py). */

/* bytes of workspace for n_images images of height x width; 0 for invalid sizes */
uint64_t nsa_image_metrics_workspace(uint32_t n_images, uint32_t height, uint32_t width);

/* ssim_mean[n_images], sq_err_sum[n_images] (device, float64); ssim_map may be NULL (no map). */
int nsa_image_metrics(const float *pred, const float *gt, uint32_t n_images, uint32_t height, uint32_t width, void *workspace,
                      double *ssim_mean, double *sq_err_sum, float *ssim_map, nsa_stream_t stream);

/* ---- Section 10: depth fusion into a dense TSDF volume (csrc/tsdf_fuse.hip) ---------------------------------- */

/* A dense truncated-signed-distance volume over an axis-aligned box: nx * ny * nz voxels, voxel (x, y, z) at
 * i = (x * ny + y) * nz + z -- the layout nsa_marching_cubes_* reads -- in three device arrays owned by the caller:
 * tsdf[nx * ny * nz] and weight[same] fp32, and colour, fp32, PLANAR: channel c of voxel i at colour[c * nx * ny * nz + i]
 * (may be NULL: no colour).  Planar because the integration kernel runs its lanes along z: every load and store of the state
 * is then one contiguous run of 4-byte words per wave, which the interleaved form (12-byte stride) is not.  A fresh volume is
 * all zeros (weight 0 = never observed).  nx * ny * nz <= 2^31.  The centre of voxel (x, y, z) is
 *   c_a = origin_a + voxel_length * ((float)i_a + 0.5f),   a = x, y, z. */
typedef struct nsa_tsdf_volume {
    float *tsdf, *weight, *colour;
    uint32_t nx, ny, nz;
    float origin[3];     /* the box's lower corner (NOT the centre of voxel 0), finite                                    */
    float voxel_length;  /* finite, > 0                                                                                   */
    float sdf_trunc;     /* finite, > 0, and 1.0f / sdf_trunc finite                                                      */
} nsa_tsdf_volume_t;

/* Integrate n depth frames IN ORDER k = 0 .. n-1: the running average of the projective truncated signed distance, the rule of
 * uniform TSDF integration (open3d's ScalableTSDFVolume::Integrate as preprocess/get_mesh_7scenes.py drives it, restated; this
 * statement is the contract).  depth[n, H, W] fp32, z-depth along the camera axis in the volume's units; rgb[n, H * W, 3] fp32
 * (required when the volume has colour, ignored otherwise, may then be NULL); w2c[n, 3, 4] fp32 world-to-camera rows
 * (R_r0 R_r1 R_r2 t_r); K[n or 1][4] = (fx, fy, cx, cy) fp32, one per frame when K_per_frame is non-zero, else one for all.
 * All fp32, every operation rounded on its own (no FMA contraction), IEEE division.  Per voxel and frame k:
 *   p_r  = ((R_r0 * c_x + R_r1 * c_y) + R_r2 * c_z) + t_r,   r = 0, 1, 2                 (camera frame)
 *   skip unless p_2 > 0
 *   u_f  = ((p_0 * fx) / p_2 + cx) + 0.5f ;  v_f = ((p_1 * fy) / p_2 + cy) + 0.5f        (pixel centres at integer (u, v))
 *   skip unless 0 <= u_f < (float)W and 0 <= v_f < (float)H ;  u = (int)u_f, v = (int)v_f
 *   d    = depth[k, v, u] ;  skip unless d > 0 and d <= depth_trunc                      (0, negative, NaN: no measurement)
 *   sdf  = d - p_2 ;  skip unless sdf > -sdf_trunc
 *   x    = sdf * inv,  inv = 1.0f / sdf_trunc ;  t = x < 1.0f ? x : 1.0f
 *   den  = weight + 1.0f
 *   tsdf = (tsdf * weight + t) / den ;  colour_c = (colour_c * weight + rgb[k, v * W + u, c]) / den ;  weight = den
 * ("skip" leaves the voxel's state untouched by that frame; a comparison with a NaN operand is false.)  Every voxel coordinate
 * is formed from its index as above, so the result does not depend on how the kernel maps threads to voxels, and n frames in
 * one call equal n calls of one frame bit for bit.  The kernel keeps a voxel's state in registers over the whole batch (one
 * read and one write of the state per call) and skips, per brick of voxels, the frames whose frustum or depth range the brick
 * cannot meet; that test is conservative and never changes a result.
 * H, W < 2^24; depth_trunc > 0 (+inf: none).  frame_zmax: 33 * n floats of device workspace (the largest accepted depth of
 * each frame and its 32 partial maxima, written by two small kernels first).  n = 0 is a no-op.  Nothing is allocated or synchronised.
 * replaces the integrate loop of preprocess/get_mesh_7scenes.py (open3d ScalableTSDFVolume) on a dense box. */
int nsa_tsdf_integrate(const nsa_tsdf_volume_t *vol, const float *depth, const float *rgb, const float *w2c, const float *K,
                       int K_per_frame, uint32_t n, uint32_t H, uint32_t W, float depth_trunc, float *frame_zmax,
                       nsa_stream_t stream);

/* Colour of the volume at m arbitrary points (mesh vertices): points[m, 3] -> out[m, 3], fp32, every operation rounded on its own.
 *   g_a = (p_a - origin_a) / voxel_length - 0.5f ;  b_a = floorf(g_a) ;  f_a = g_a - b_a        (voxel-centre grid coordinate)
 *   corner (dx, dy, dz) in {0, 1}^3 is voxel (b_x + dx, b_y + dy, b_z + dz) with
 *   w = (wx * wy) * wz,  wa = da ? f_a : 1.0f - f_a ;  it SURVIVES when it lies inside the volume and its weight > 0
 *   s = sum of w, a_c = sum of w * colour_c over the surviving corners, added in the order dx outermost, dz innermost
 *   out_c = a_c / s when s > 0, else 0 (also for a point with a non-finite coordinate or outside every cell). */
int nsa_tsdf_sample_colour(const nsa_tsdf_volume_t *vol, const float *points, uint64_t m, float *out, nsa_stream_t stream);

/* ---- Section 11: mesh components (connected components of a triangle mesh and their statistics; DESIGN 4j, csrc/mesh_clean.hip) - */

/* Labelling.  faces[n_faces, 3] int32 over n_verts vertices; n_verts, n_faces < 2^31.  A face is VALID when its three indices lie
 * in [0, n_verts); a valid face connects its three vertices (a degenerate one, (a, a, b), too); an invalid face connects nothing.
 * A component is an equivalence class of vertices under "used by a common valid face", closed transitively, and its LABEL is
 * the smallest vertex index in it.  Connectivity is by index only: coordinates play no part, and unwelded duplicates are
 * different vertices (trimesh with process=False, as eval_rec.py loads meshes).
 *   vertex_label[n_verts]  the label of the vertex's component, -1 for a vertex no valid face uses
 *   face_label[n_faces]    the label of the face's vertices, -1 for an invalid face
 *   totals[3]              (uint64, device) {components, referenced vertices, status}; the caller reads them once to size the
 *                          statistics, as it reads the totals of nsa_marching_cubes_count
 * The outputs are a function of the face list alone.  Inside, a lock-free union-find reaches the fixed point with compare-and-swap
 * (parent[x] <= x throughout, larger root hooked under smaller), so atomics are used but decide nothing in the output.  Every
 * device loop also has a step cap (a walk to the root: n_verts steps; hook retries: n_verts); a cap that trips sets a bit of
 * status (1: walk, 2: hook) and the labels are then meaningless.  status is 0 for every input unless the implementation is
 * wrong; the entry point does not synchronise, so the caller sees it when it reads the totals.
 * Departure from trimesh's split (code/utils/viz.py:136-141), which joins faces that share an EDGE: here faces that share a
 * VERTEX are joined, so a component here is a union of trimesh's; the two agree on manifold meshes.
 * n_verts = n_faces = 0 is a no-op that returns 0 and launches nothing.  n_faces = 0 with n_verts > 0 writes every
 * vertex_label = -1 and totals = {0, 0, 0}.  Nothing is allocated or synchronised; the workspace belongs to the caller. */

/* bytes of workspace for n_verts (>= 1) vertices; 0 for an invalid count */
uint64_t nsa_mesh_components_workspace(uint32_t n_verts);

int nsa_mesh_components(const int32_t *faces, uint32_t n_faces, uint32_t n_verts, void *workspace, int32_t *vertex_label,
                        int32_t *face_label, uint64_t *totals, nsa_stream_t stream);

/* Statistics, after nsa_mesh_components on the same mesh, with n_components = totals[0] (<= n_faces).  The components in
 * ascending label order have RANK c = 0 .. n_components - 1:
 *   label[C] int32      the label of component c
 *   n_faces[C] int32    its valid faces
 *   n_verts[C] int32    its vertices
 *   area[C] float64     the sum of its face areas a_f = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz) of Section 8 (the same device
 *                       function); a face that touches a vertex with a non-finite coordinate counts 0
 *   lo[C, 3], hi[C, 3]  fp32 minimum / maximum of its vertices per axis, a non-finite coordinate skipped (per axis); -0 orders
 *                       below +0; (+inf, -inf) when none is finite
 *   vertex_comp[n_verts], face_comp[n_faces] int32   the rank of the element's component, -1 where its label is -1
 * Order of the area sum: the faces are argsorted stably by rank (equal ranks keep their index order); within each aligned block
 * of 1024 sorted positions the run of a component is summed left to right from 0.0; a component's total is its first run plus
 * the runs at the heads of the following blocks, added in block order.  Counts and boxes are integer sums / minima / maxima
 * (the box on an order-preserving integer image of the fp32 value) and do not depend on any order: every output is
 * bit-reproducible.  A count other than the labelling's gives -1 ranks for the components past it and never writes out of
 * bounds.  n_components = 0 writes only the two rank arrays.  Nothing is allocated or synchronised. */

/* bytes of workspace; 0 for invalid counts (n_verts = 0, a count >= 2^31, n_components > n_faces or > n_verts) */
uint64_t nsa_mesh_component_stats_workspace(uint32_t n_verts, uint32_t n_faces, uint32_t n_components);

int nsa_mesh_component_stats(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                             const int32_t *vertex_label, const int32_t *face_label, uint32_t n_components, void *workspace,
                             int32_t *label, int32_t *n_faces_out, int32_t *n_verts_out, double *area, float *lo, float *hi,
                             int32_t *vertex_comp, int32_t *face_comp, nsa_stream_t stream);

/* ---- Section 12: mesh rasterisation and visibility (z-buffered images of a triangle mesh; DESIGN 4k, csrc/mesh_raster.hip) ---- */

/* What code/utils/viz.py leaves to open3d's OpenGL window, and the depth image of a mesh that visibility culling needs.  There is no
 * renderer to be bit-equal to, so this statement is the contract: all floating point is fp32, every operation rounded on its own
 * (no FMA contraction), IEEE division and square root; all coverage arithmetic is exact int64.  tests/raster_ref.py restates it in
 * numpy and the kernels equal it bit for bit.
 *
 * Inputs.  verts[V, 3] fp32, faces[F, 3] int32, and a batch of n views: w2c[n, 3, 4] fp32 world-to-camera rows (the caller inverts
 * camera-to-world in float64 and rounds once), K[n or 1][4] = (fx, fy, cx, cy), an image of H x W pixels whose centres sit at
 * integer (i, j) = (column, row) -- the conventions of Section 10 -- and near.  1 <= H, W <= NSA_RASTER_GUARD_PIXELS;
 * 0 < near < NSA_RASTER_FAR; V, F, F + P < 2^31.
 *
 * Vertex v in a view:
 *   p_r = ((R_r0 * v_x + R_r1 * v_y) + R_r2 * v_z) + t_r,  r = 0, 1, 2
 *   DEPTH test   near < p_2 <= NSA_RASTER_FAR                                  (false for NaN)
 *   x = (p_0 * fx) / p_2 + cx ;  y = (p_1 * fy) / p_2 + cy
 *   GUARD test   |x| <= G and |y| <= G,  G = NSA_RASTER_GUARD_PIXELS            (false for NaN)
 *   X = (int32)rint(x * 256.0f), Y likewise: a grid of 1/256 pixel (round half to even; x * 256 is exact).  |X| <= 2^22, so every
 *   product of two coordinate differences is below 2^47 and the edge functions below are exact in int64.
 *   Against the exact projection of the fp32 inputs, with u = 2^-24, m_r = |R_r0 v_x| + |R_r1 v_y| + |R_r2 v_z| + |t_r|:
 *     |x - x_exact| <= u * (4 fx m_0 / p_2 + |x - cx| * (2 + 4 m_2 / p_2) + |x|)  to first order (four roundings in p_0 and in p_2,
 *     one each in the product, the quotient and the sum), so |X - 256 x_exact| <= 1/2 + 256 times that: below 0.6 units
 *     inside a 340 x 600 image of a room at a focal length of 300 pixels.
 * Face.  Its indices are first rotated so that the smallest comes first, (A, B, C), keeping the winding: the image of a face depends
 * on its vertex set and winding, not on which vertex the file lists first.  A face is DRAWN in a view unless, tested in this order:
 *   1 an index lies outside [0, V) (Section 11's validity)    2 a vertex fails the DEPTH test (NaN, behind the camera, across near)
 *   3 a vertex fails the GUARD test    4 area2 = (B_X - A_X)(C_Y - A_Y) - (B_Y - A_Y)(C_X - A_X) = 0
 *   5 cull_backface is set and area2 > 0 (the normal (B - A) x (C - A) points away from the camera; x right, y down, z forward)
 * A face that is not drawn is skipped WHOLE and counted: totals[c] += 1 per (face, view) with c the number above, totals[0] for drawn.
 * DEPARTURE: there is no near-plane clipping; a face with one vertex behind near vanishes instead of being cut.
 * When area2 < 0, B and C (and their 1/z) are exchanged and area2 negated, so that orient(A, B, C) > 0 below.
 * Coverage of pixel centre P = (256 i, 256 j), with orient(a, b, p) = (b_X - a_X)(p_Y - a_Y) - (b_Y - a_Y)(p_X - a_X) in int64:
 *   w_0 = orient(B, C, P), w_1 = orient(C, A, P), w_2 = orient(A, B, P)          (w_0 + w_1 + w_2 = area2)
 *   edge a -> b OWNS the centres exactly on it when b_Y < a_Y, or b_Y = a_Y and b_X > a_X (left and top edges: the top-left rule)
 *   covered  <=>  for each k: w_k > 0, or w_k = 0 and its edge owns.
 *   Two drawn faces on opposite sides of a shared edge run it in opposite directions, exactly one direction owns, and w is exact:
 *   a centre on the edge belongs to exactly one of them.  Candidates are the centres inside the bounding box of the snapped vertices,
 *   clamped to the image: i from max(0, ceil(min X / 256)) to min(W - 1, floor(max X / 256)), j likewise.
 * Depth at a covered pixel:
 *   l_k = (float)w_k / (float)area2      (int64 -> fp32 round to nearest, then one division)
 *   z_inv = (l_0 * (1.0f / p_2A) + l_1 * (1.0f / p_2B)) + l_2 * (1.0f / p_2C) ;  depth = 1.0f / z_inv       (z-depth, as Section 10)
 *   Since 1/z is affine on the screen, the only error beyond rounding is the snap: every snapped vertex lies within
 *   s = 1/512 pixel (plus the projection error above) of its projection per axis, so z_inv is the plane's exact 1/z at a point
 *   within s of the centre, and |depth - exact| <= depth * exact * (|d(1/z)/di| + |d(1/z)/dj|) * s  plus a few ulp.
 * Winner.  zbuf[n, H, W] uint64, empty = all ones.  key = (uint64)(bits of depth) << 32 | id with id = the face index; every
 * covered (face, pixel) does one unsigned 64-bit atomic minimum.  depth is positive and finite, so keys order as depths, and ties in
 * depth go to the smaller id.  The minimum is independent of arrival order: the image is a function of the inputs alone.
 * Points.  points[P, 3] fp32 drawn as squares of point_size (1 .. NSA_RASTER_MAX_POINT_SIZE) pixels with id = F + index: a point that
 * passes DEPTH and GUARD covers the centres with X - h <= 256 i < X + h and Y - h <= 256 j < Y + h, h = 128 * point_size, all at
 * depth = p_2 (totals[9] drawn, totals[10] skipped, per (point, view)).
 * Large faces.  A drawn face with more than large_threshold candidate centres is cut into (face, view, 64 x 64 screen tile) items in
 * a queue in the workspace and drawn by a second kernel, one wave per item; 0 sends every face that way, 0xFFFFFFFF none.  Both
 * ways apply the same rule, so the image does not depend on large_threshold or queue_capacity (a face whose items do not fit the
 * queue is drawn the first way).  totals[6] = atomic minima issued = covered (face or point, pixel) pairs, totals[7] = (face, view)
 * pairs that asked for the queue, totals[8] = items queued; [7] and [8] depend on large_threshold, [8] on the capacity, nothing else does.
 * Nothing is allocated or synchronised; zbuf, totals and the workspace belong to the caller. */
#define NSA_RASTER_GUARD_PIXELS 16384
#define NSA_RASTER_FAR 1e30f
#define NSA_RASTER_MAX_POINT_SIZE 64
#define NSA_RASTER_TOTALS 12

typedef struct nsa_raster_views {
    const float *w2c;    /* [n, 3, 4]                                                                                     */
    const float *K;      /* [n, 4] when K_per_view is non-zero, else [1, 4]                                               */
    uint32_t n;          /* views in the batch, 1 .. 2^20, n * H * W < 2^40                                               */
    int K_per_view;
    uint32_t H, W;
    float near;
} nsa_raster_views_t;

/* bytes of workspace for a queue of queue_capacity items (16 bytes each, after a 16-byte header) */
uint64_t nsa_mesh_raster_workspace(uint32_t queue_capacity);

/* Faces and points into zbuf for a batch of views.  clear non-zero: zbuf is first set to all ones and totals[NSA_RASTER_TOTALS]
 * (uint64, device) to zero; zero: both are accumulated into, so several calls can draw into one image (ids are the caller's to
 * keep apart).  points may be NULL with n_points = 0, faces with n_faces = 0. */
int nsa_mesh_raster(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const float *points,
                    uint32_t n_points, uint32_t point_size, const nsa_raster_views_t *views, int cull_backface, int clear,
                    uint32_t large_threshold, void *workspace, uint32_t queue_capacity, uint64_t *zbuf, uint64_t *totals,
                    nsa_stream_t stream);

/* Resolve, per pixel of a finished zbuf; every output [n, H, W (, 3)] is optional (NULL), at least one is required:
 *   face_id int32   the winner's id (a point: F + index), -1 where empty
 *   depth fp32      the key's depth, 0 where empty (Section 10's "no measurement": the image feeds nsa_tsdf_integrate unchanged)
 * and for a face, recomputed from its id and the same integers (a point: normal 0, shade 1, colour = palette[point_colour[index]],
 * 0 when that index is outside [0, n_palette); empty: all 0):
 *   normal   c = (B - A) x (C - A) of the rotated, unswapped face, each component a difference of two products;
 *            len = sqrt((c_x c_x + c_y c_y) + c_z c_z); n = c / len, or 0 unless 0 < len <= 3e38.  With flip_to_camera, n is negated
 *            for a face with area2 > 0, so that every normal faces the camera by the same integer test that culls.
 *   colour   q_k = l_k * (1.0f / p_2k); colour_c = ((q_0 * c_Ac + q_1 * c_Bc) + q_2 * c_Cc) / ((q_0 + q_1) + q_2) with colours[V, 3]
 *            (perspective-correct; B and C as exchanged above); 0 when colours is NULL
 *   shade    the headlight term |n_c . d|: n_c,r = (R_r0 n_x + R_r1 n_y) + R_r2 n_z (before the flip), d_x = ((float)i - cx) / fx,
 *            d_y = ((float)j - cy) / fy, shade = |((n_c0 * d_x + n_c1 * d_y) + n_c2) / sqrt((d_x d_x + d_y d_y) + 1.0f)|. */
int nsa_mesh_raster_resolve(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const float *colours,
                            const int32_t *point_colour, uint32_t n_points, const float *palette, uint32_t n_palette,
                            const nsa_raster_views_t *views, const uint64_t *zbuf, int flip_to_camera, int32_t *face_id,
                            float *depth, float *normal, float *colour, float *shade, nsa_stream_t stream);

/* Visibility of faces in the finished views of zbuf.  A vertex is SEEN in a view when it passes DEPTH and GUARD, 0 <= x <= W - 1 and
 * 0 <= y <= H - 1, and p_2 <= (1.0f + rel) * z_max, z_max = the largest zbuf depth over the four centres (i0, j0), (i1, j0), (i0, j1),
 * (i1, j1), i0 = (int)floor(x), i1 = min(i0 + 1, W - 1), j likewise; an empty pixel counts as +inf.  A face with valid indices is
 * visible in a view when any (NSA_VISIBLE_ANY) or all three (NSA_VISIBLE_ALL) of its vertices are seen in it; NSA_VISIBLE_FRUSTUM is
 * ANY without the depth comparison (zbuf may be NULL).  visible[F] uint8 gets a plain store of 1 for a face visible in some view of the
 * batch and is otherwise left alone, so calls over several batches OR into it (the caller zeroes it first).  Visibility is decided at
 * vertices against the depth image because a face smaller than a pixel covers no centre and would never appear in face_id.
 * 0 <= rel <= 1. */
#define NSA_VISIBLE_ANY 0
#define NSA_VISIBLE_ALL 1
#define NSA_VISIBLE_FRUSTUM 2
int nsa_mesh_visible(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const nsa_raster_views_t *views,
                     const uint64_t *zbuf, int mode, float rel, uint8_t *visible, nsa_stream_t stream);

/* ---- Section 13: optical-flow ground truth from depth and poses (csrc/flow_cues.hip) ---- */

/* What the reference reads from its *_pair directories (preprocess/extract_flows.py: GMFlow and a forward-backward consistency
 * check; code/training/volsdf_train.py:312-361: the edge graph, the files and the per-iteration gather).  With depth frames and
 * poses the flow between two frames is geometry, and this statement is the contract (tests/flow_ref.py restates it in float64).
 * Conventions are Section 10's: pixel centres at integer (u, v) = (column, row), z-depth, K rows (fx, fy, cx, cy).  All arithmetic is
 * float64 per pixel and every output is rounded once on its store.  Each entry point is ONE launch over all its edges or pairs, of
 * fewer than 2^24 workgroups of 256 lanes (a lane owns 1 to 4 pixels or one sample), more is NSA_EBADARG;
 * nothing is allocated or synchronised; empty work (no edges, no pairs, n = 0) returns 0 without a launch.
 *
 * Induced flow.  depth[n_frames, H, W] fp32; K[n_frames or 1][4] float64; rel[n_edges, 3, 4] float64 rows [R_e | t_e] of
 * inv(c2w_j) * c2w_i, composed by the caller in float64, i = src[e], j = dst[e] (int32, device).  Pixel (u, v) of frame i, depth d:
 *   X = ((u - cx_i) / fx_i * d, (v - cy_i) / fy_i * d, d) ;  Y = R_e X + t_e
 *   flow[e, v, u] = (fx_j * Y_0 / Y_2 + cx_j - u,  fy_j * Y_1 / Y_2 + cy_j - v)            [n_edges, H, W, 2] fp32
 *   valid[e, v, u] = isfinite(d) and d > 0 and Y_2 > near                                  [n_edges, H, W] uint8; invalid: flow (0, 0)
 * Leaving the image does not make a pixel invalid (that is the consistency rule's to find).  An edge whose src or dst lies outside
 * [0, n_frames) reads nothing and is invalid everywhere.  H * W < 2^31, 0 <= near < inf. */
int nsa_flowcue_induced(const float *depth, uint32_t n_frames, uint32_t H, uint32_t W, const double *K, int K_per_frame,
                        const double *rel, const int32_t *src, const int32_t *dst, uint32_t n_edges, double near, float *flow,
                        uint8_t *valid, nsa_stream_t stream);

/* Forward-backward consistency (GMFlow's rule, as extract_flows.py applies it).  fwd, bwd [n_pairs, H, W, 2] fp32; per pixel p = (u, v):
 *   mag = |fwd(p)| + |bwd(p)|                                    (both at the SAME pixel: the rule's own quirk, kept)
 *   wb  = bilinear sample of bwd at p + fwd(p) in pixel coordinates, taps outside the image count as zero
 *   fwd_occ(p) = |fwd(p) + wb| > alpha * mag + beta              1 = occluded; bwd_occ likewise with the roles exchanged
 * With validity maps (both or neither, [n_pairs, H, W] uint8) a pixel is also occluded when it is itself invalid, or when the bilinear
 * sample of the partner's invalidity map (1 - valid, zero outside the image) at its landing point exceeds 1e-3.  A non-finite landing
 * point reads nothing.  H, W >= 2, H * W < 2^31, alpha and beta finite and >= 0. */
int nsa_flowcue_consistency(const float *fwd, const float *bwd, const uint8_t *fwd_valid, const uint8_t *bwd_valid, uint32_t n_pairs,
                            uint32_t H, uint32_t W, double alpha, double beta, uint8_t *fwd_occ, uint8_t *bwd_occ,
                            nsa_stream_t stream);

/* The per-iteration gather (select_flow_uv): flows[n_edges, n_pixels, 2] fp32 and masks[n_edges, n_pixels] bytes resident on the
 * device, sampling_idx[b, n] and idii[n_edges] int64:
 *   out_flow[e, k] = flows[e, s], out_mask[e, k] = masks[e, s] != 0,  s = sampling_idx[idii[e], k]
 * and flow 0, mask 0 when s lies outside [0, n_pixels) or idii[e] outside [0, b): nothing is ever read out of range.
 * 0 < n_pixels < 2^31. */
int nsa_flowcue_select(const float *flows, const uint8_t *masks, uint32_t n_edges, uint64_t n_pixels, const int64_t *sampling_idx,
                       uint32_t b, uint32_t n, const int64_t *idii, float *out_flow, uint8_t *out_mask, nsa_stream_t stream);

/* ---- Section 14: closest point on a triangle mesh (csrc/mesh_closest.hip) ---- */

/* What trimesh.proximity.closest_point gives eval_rec.py:120-129 (distance_p2m): for every query point the closest point of a
 * triangle mesh, the distance to it and the face it lies on.  verts[n_verts, 3] fp32, faces[n_faces, 3] int32, queries[n_queries, 3]
 * fp32, all C-contiguous; counts below 2^31.  tests/p2m_ref.py restates this statement in numpy float64.
 *
 * Per (query q, face (a, b, c) in the order listed).  All arithmetic is float64 on the fp32 inputs, every operation rounded on its own
 * (no FMA contraction), divisions are IEEE, and dot(u, v) = (u_x * v_x + u_y * v_y) + u_z * v_z:
 *   ab = b - a ; ac = c - a ; ap = q - a ; bp = q - b ; cp = q - c                                        (component by component)
 *   d1 = dot(ab, ap) ; d2 = dot(ac, ap) ; d3 = dot(ab, bp) ; d4 = dot(ac, bp) ; d5 = dot(ab, cp) ; d6 = dot(ac, cp)
 *   vc = d1 * d4 - d3 * d2 ; vb = d5 * d2 - d1 * d6 ; va = d3 * d6 - d5 * d4
 * The region classification of Ericson, Real-Time Collision Detection 5.1.5, in the book's order; (s, t) is that of the FIRST line
 * whose test holds:
 *   1 vertex a   d1 <= 0 and d2 <= 0                         s = 0 ; t = 0
 *   2 vertex b   d3 >= 0 and d4 <= d3                        s = 1 ; t = 0
 *   3 edge ab    vc <= 0 and d1 >= 0 and d3 <= 0             s = d1 / (d1 - d3) ; t = 0
 *   4 vertex c   d6 >= 0 and d5 <= d6                        s = 0 ; t = 1
 *   5 edge ac    vb <= 0 and d2 >= 0 and d6 <= 0             s = 0 ; t = d2 / (d2 - d6)
 *   6 edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)) ; s = 1 - w ; t = w
 *   7 interior   otherwise                                   e = 1 / ((va + vb) + vc) ; s = vb * e ; t = vc * e
 *   p = (a + s * ab) + t * ac ;  r = q - p ;  d2(q, face) = (r_x * r_x + r_y * r_y) + r_z * r_z
 *
 * Skipped faces.  A face is skipped -- never returned -- and counted in totals[3] (uint32, device; may be NULL) under the FIRST cause
 * that holds:  totals[0] an index lies outside [0, n_verts);  totals[1] a vertex has a non-finite coordinate;  totals[2] ab x ac,
 * (ab_y * ac_z - ab_z * ac_y, ab_z * ac_x - ab_x * ac_z, ab_x * ac_y - ab_y * ac_x) in float64, is exactly (0, 0, 0).  Dropping
 * zero-area faces changes the surface on a set of measure zero only and keeps 1 / 0 out of line 7.
 *
 * Result per query.  The winner is the face with the smallest d2 over the faces not skipped (a NaN d2 never wins), ties to the LOWEST
 * face index:  face_idx = its index;  d2 = its float64 d2;  closest (may be NULL) = its p, rounded once to fp32 on the store.
 * A query with a non-finite coordinate gives (-1, NaN); a mesh without a usable face gives (-1, +inf); closest is NaN in both cases.
 * The result is a function of (queries, verts, faces) alone and equals a brute force over all faces in this operation order on every
 * input: the index only skips work.  No atomic takes part (the skip counts are a block reduction).
 *
 * Index: Section 8's grid -- bulk quantiles of a strided subsample, near-cubic cells, border clamping -- over the fp32
 * centroids fp32(((a + b) + c) / 3) of the usable faces, at most min(2 * n_faces, 2^22) cells, each with the union of its faces'
 * boxes.  A face longer than 2 cells on an axis, or with sigma = Lmax^2 / |ab x ac|^2 (Lmax its longest edge) above 2^16 / hmax^2
 * (hmax the longest cell edge), or with its centroid more than 256 cells outside the grid, is kept on a separate list that every
 * query walks (the large-face queue of Section 12 is the precedent).  Margins of the conservative bounds, each against the rounding of the quantity it bounds:
 *   boxes        every bound moved outwards by 2^-40 of the larger bound's magnitude on that axis, then rounded outwards to fp32:
 *                (a + s * ab) + t * ac is within 2^-50 of that magnitude of the exact combination;
 *   (s, t)       in line 7 va, vb, vc are differences of products of magnitude L^2 D^2 (L the longest edge, D the largest distance
 *                from q to a vertex of the face), each within 40 * 2^-53 * L^2 D^2 of its exact value, while their exact sum is
 *                |ab x ac|^2; so p lies within rho * L of the triangle, rho = 2^-43 * sigma * D^2 (a factor 6 above that count), as
 *                long as rho <= 1/4.  Lines 1-6 give s, t in [0, 1] by the monotonicity of rounding;
 *   skip rule    a box (of a face, a cell, or of everything beyond a ring) at distance g is skipped only when rho <= 1/4 and
 *                (g - rho * diag)^2 > best * (1 + 2^-40), with diag >= L; the 2^-40 is far above the float64 rounding of g^2.  With
 *                rho > 1/4 nothing is skipped: a brute force.  Grid faces share one rho per query: sigma <= 2^16 / hmax^2,
 *                L <= 2 |h|, and D <= the distance to the far corner of the grid faces' box, which is the box of all usable faces
 *                clipped to 259 cells around the grid (a centroid at most 256 cells outside, a box of at most 2 cells, one cell
 *                of margin).  A grid measures at most 2^10 cells a side, so rho <= 2^-27 * 3 * (1024 + 518)^2 = 0.053 for every
 *                query inside that box, and reaches 1/4 when its far corner is 2^12.5 cells away.  A stray component farther out
 *                than 256 cells goes on the list and costs every query a box test per face, not the pruning.  A listed face uses
 *                its own sigma and D <= g + diag;
 *   ring stop    per axis and side the cell plane at the ring, less 2^-9 cell (the fp32 cell index is off by less than 2^-12 cell),
 *                less 2 cells and the padding (how far a grid face reaches beyond its centroid), combined with the query's
 *                distance to the grid faces' box on the other axes, under the skip rule.
 * The reach is the bound the construction gives (a box of at most 2 cells around a centroid inside it), not the largest extent found
 * in the mesh: that would take a reduction over the faces for a stop rule at most 2/3 cell tighter.
 * Worst cases: every face in one cell, every face on the list, or rho > 1/4 (a query 2^12.5 cells away) -- all are
 * a brute force, slow and never wrong.
 *
 * Workspace: a function of n_faces alone, for any mesh:  with B = min(2 * n_faces, 2^22) and every array rounded up to 256 bytes,
 *   256 + 4 (B + 3) + 24 B + 32 F + 5 * 4 F + 2^18   bytes   (<= 108 * n_faces + 2^18 + 3072).
 * Nothing is allocated or synchronised; arguments are checked before the device is touched (NSA_EBADARG: a NULL array, n_verts = 0,
 * n_faces = 0, a count of 2^31 or more); the index buffer belongs to the caller.  The index refers to the mesh by face number: the
 * verts and faces given to nsa_tri_query are those given to nsa_tri_build, unchanged. */

/* bytes of the index buffer for n_faces (>= 1) faces; 0 for an invalid count */
uint64_t nsa_tri_workspace(uint32_t n_faces);

/* Build the index into `index` (nsa_tri_workspace(n_faces) bytes, device, 256-byte aligned); totals[3] as above (may be NULL). */
int nsa_tri_build(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, void *index, uint32_t *totals,
                  nsa_stream_t stream);

/* face_idx[n_queries] int32, d2[n_queries] float64, closest[n_queries, 3] fp32 or NULL.  n_queries = 0 returns 0 without a launch. */
int nsa_tri_query(const void *index, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                  const float *queries, uint32_t n_queries, int32_t *face_idx, double *d2, float *closest, nsa_stream_t stream);

/* The same query; evaluated[n_queries] uint32 (may be NULL) receives how many faces went through the full evaluation for each query
 * -- a measurement of the index (tools/bench_mesh_closest.py), not part of the answer. */
int nsa_tri_query_counted(const void *index, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                          const float *queries, uint32_t n_queries, int32_t *face_idx, double *d2, float *closest,
                          uint32_t *evaluated, nsa_stream_t stream);

/* ---- Section 15: signed distance to a triangle mesh and range-limited queries (csrc/mesh_sdf.hip) ---- */

/* Section 14's query with a sign and with a bound.  tests/sdf_ref.py restates this statement in numpy float64.
 *
 * Winner.  Everything about the winner is Section 14's, unchanged: the usable faces and the three skip causes, float64 with every
 * operation rounded on its own, the order of the region tests, the smallest d2 with ties to the lowest face index, p rounded once to
 * fp32 on the store.  face_idx, d2 and closest equal nsa_tri_query's bit for bit (where the bound lets them through).
 *
 * Feature.  The line of Section 14's classification that gave the winner's (s, t):
 *   0 interior   1 vertex a   2 vertex b   3 edge ab   4 vertex c   5 edge ac   6 edge bc   -1 no winner
 *
 * Adjacency is by vertex index over a second int32 array adjacency_faces[n_faces, 3], with the numbering of `faces`, in which
 * coincident vertices share an index (TriIndex fills it with `faces` after welding vertices whose fp32 coordinates are equal,
 * -0 = +0).  A face CONTRIBUTES when it is usable under Section 14 and its three adjacency indices lie in [0, n_verts); an adjacency
 * index outside that range is never dereferenced.
 *
 * Unit face normal, float64, divisions and the square root IEEE:
 *   n_g = (ab x ac) / sqrt((x * x + y * y) + z * z),  (x, y, z) = ab x ac in Section 14's component order.
 * Pseudo-normal N and weight W of the winner f's feature (Baerentzen & Aanaes 2005), sums from 0 in ascending g, N component by
 * component as N + alpha_g * n_g (N + n_g on an edge):
 *   interior      N = n_f, W = 1 (whether f contributes or not)
 *   edge {i, j}   N = the sum of n_g over the contributing faces g that list both i and j (each once), W = their count: one on a
 *                 boundary edge, all of them on a non-manifold edge
 *   vertex i      N = the sum of alpha_g * n_g over the contributing corners at i, W = the sum of alpha_g,
 *                 alpha_g = atan2(|u x w|, dot(u, w)), u and w the float64 edges from that corner to the next and to the previous
 *                 corner of g (a -> b, c ; b -> c, a ; c -> a, b)
 * with i, j the adjacency indices of f's corners.  Sign: e = q - p with p in float64 (before the store);  sign = -1 when
 * dot(e, N) < 0, else +1 -- so d2 = 0, dot(e, N) = 0 and N = 0 all give +1 -- and a non-zero `flip` negates it.  Positive is the side
 * ab x ac points to.  For a closed manifold mesh this is outside / inside exactly; for an open mesh it is the side of the nearest
 * surface element.  Two coincident faces of opposite winding give N = 0 on their interior: +1.
 *
 * Bound.  max_d2 in float64; +inf = unbounded; NaN or negative is NSA_EBADARG.  The answer is the unbounded answer when its
 * d2 <= max_d2 (equality included), otherwise (face -1, d2 +inf, closest NaN, feature -1, sign +1 before flip).  A non-finite query
 * gives (-1, NaN, NaN, -1, +1 before flip).  The walk starts from the float64 after max_d2 as the distance to beat, so every skip
 * rule of Section 14 prunes against the bound from the first cell on: the cost is set by the bound, not by the distance to the surface.
 *
 * What is bit-exact: face_idx, d2, closest, feature.  N and W are not (atan2 is not the same function in every maths library); the
 * tests hold |N - N_ref| to 2^-40 W per component and the sign wherever |dot(e, N)| > 2^-36 |e| W.  The results are a function of the
 * inputs alone: the adjacency is a stable sort, no atomic takes part.
 *
 * Adjacency workspace, a function of (n_verts, n_faces) alone, every array rounded up to 256 bytes:
 *   4 (V + 2) + 5 * 12 F + 2^18   bytes   (<= 4 * n_verts + 60 * n_faces + 2^18 + 2048);   n_faces <= (2^31 - 1) / 3.
 * A query whose winner's feature is a vertex of k contributing corners walks k of them; an edge walks the shorter of its two
 * endpoints' lists.  Slow at a vertex of very high valence and never wrong.  nsa_tri_workspace and the index are unchanged. */

/* bytes of the adjacency buffer; 0 for an invalid count */
uint64_t nsa_tri_adjacency_workspace(uint32_t n_verts, uint32_t n_faces);

/* Build the vertex -> face lists into `adjacency` (device, 256-byte aligned) from the mesh the index was built on and adjacency_faces. */
int nsa_tri_adjacency_build(const float *verts, uint32_t n_verts, const int32_t *faces, const int32_t *adjacency_faces,
                            uint32_t n_faces, void *adjacency, nsa_stream_t stream);

/* face_idx[n_queries] int32, d2[n_queries] float64, closest[n_queries, 3] fp32 or NULL, feature[n_queries] int8, sign[n_queries] int8.
 * n_queries = 0 returns 0 without a launch. */
int nsa_tri_signed_query(const void *index, const void *adjacency, const float *verts, uint32_t n_verts, const int32_t *faces,
                         const int32_t *adjacency_faces, uint32_t n_faces, const float *queries, uint32_t n_queries, double max_d2,
                         int flip, int32_t *face_idx, double *d2, float *closest, int8_t *feature, int8_t *sign, nsa_stream_t stream);

/* The same query; each may be NULL: normal[n_queries, 3] and weight[n_queries] float64 receive N and W (for the tests),
 * evaluated[n_queries] and cells[n_queries] uint32 the faces fully evaluated and the grid cells looked at (empty ones included). */
int nsa_tri_signed_query_counted(const void *index, const void *adjacency, const float *verts, uint32_t n_verts, const int32_t *faces,
                                 const int32_t *adjacency_faces, uint32_t n_faces, const float *queries, uint32_t n_queries,
                                 double max_d2, int flip, int32_t *face_idx, double *d2, float *closest, int8_t *feature, int8_t *sign,
                                 double *normal, double *weight, uint32_t *evaluated, uint32_t *cells, nsa_stream_t stream);

/* nsa_tri_query_counted under the bound (no sign, no adjacency); evaluated and cells as above, each may be NULL. */
int nsa_tri_query_bounded(const void *index, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                          const float *queries, uint32_t n_queries, double max_d2, int32_t *face_idx, double *d2, float *closest,
                          uint32_t *evaluated, uint32_t *cells, nsa_stream_t stream);

/* ---- Section 16: generalised winding number of a triangle mesh (csrc/mesh_winding.hip) ---- */

/* w(q) = (1 / 4 pi) * the sum of the signed solid angles under which the faces are seen from q (Jacobson et al. 2013): 1 inside and 0
 * outside a closed mesh with outward normals, and on an open mesh a smooth field that is 1/2 across a hole's virtual closure -- the
 * inside / outside test Section 15's sign is not.  Two forms behind one entry point: the exact sum, and the hierarchical first-order
 * approximation of Barill et al. 2018 whose cost per query does not grow with n_faces.  tests/winding_ref.py restates this statement
 * in numpy float64.  verts, faces, queries as in Section 14; the tree is independent of Section 14's index.
 *
 * Faces and arithmetic.  The usable faces are exactly Section 14's.  Everything is float64 on the fp32 inputs, every operation
 * rounded on its own (no FMA contraction), dot(u, w) and u x w in Section 14's component order.
 *
 * Solid angle of face (a, b, c) from q (Van Oosterom & Strackee 1983):
 *   A = a - q ; B = b - q ; C = c - q ;  lA = sqrt(dot(A, A)) ; lB, lC alike
 *   det = dot(A, B x C)
 *   den = ((lA * lB) * lC + dot(A, B) * lC) + (dot(A, C) * lB + dot(B, C) * lA)
 *   Omega = 2 * atan2(det, den), and Omega = 0 when det == 0: a query on a vertex or in a face's plane gets a defined value.
 * A face whose ab x ac points AWAY from q contributes Omega > 0.  The open unit square in z = 0 with normals +z gives
 * w = +-(1 / pi) atan(1 / (2 h sqrt(4 h^2 + 2))) at (1/2, 1/2, -+h): 1/6 at h = 1/2.
 *
 * Tree.  lo_k = the least coordinate k over the vertices of the usable faces (-0 as +0), side = the largest of the three extents,
 * L = the smallest integer with 8 * 4^L >= F_usable, at most 10.  A usable face has centroid ((a + b) + c) / 3 and lies in the leaf cell
 *   cell_k = (uint32) min(max((centroid_k - lo_k) * (2^L / side), 0), 2^L - 1)
 * with the 3 L-bit Morton code of (cell_x, cell_y, cell_z), x the highest bit of each triple, as its key.  The faces are taken in the
 * order of a stable sort by key (ascending face index within a leaf).  A node exists for every level l in [0, L] and every distinct
 * prefix key >> 3 (L - l); its faces are contiguous in that order.  Per face n_t = (ab x ac) * 0.5 and
 * area_t = sqrt((n_x * n_x + n_y * n_y) + n_z * n_z).  Per node, every sum from +0, component by component:
 *   leaf     N = sum n_t ;  area = sum area_t ;  M = sum area_t * centroid_t   over its faces in sorted order
 *   parent   the same three sums over its children in ascending key order (a lone child is repeated bit for bit)
 *   P = M / area ;  r2 = the largest dot(v - P, v - P) over the vertices v of its faces (a maximum: the same bits in any order)
 * Nodes are numbered in pre-order, children in ascending key order.  No atomic takes part: the order of every sum is fixed by the
 * sort, and two builds give identical bits.
 *
 * Query.  S = +0 and i = 0; while i < node count, with d = P_i - q and d2 = dot(d, d):
 *   d2 > beta^2 * r2_i    S = S + dot(N_i, d) / (d2 * sqrt(d2)) ; go to the first node behind i's subtree      (accepted += 1)
 *   else, at a leaf       S = S + Omega for each of its faces in sorted order ; go to i + 1                    (evaluated += faces)
 *   else                  go to i + 1
 * w = S / (4 pi) with 4 pi = 0x1.921fb54442d18p+3, negated by a non-zero `flip`.  beta^2 = beta * beta is formed once on the host.
 * beta = +inf never accepts a node: w is the exact sum over the usable faces in sorted order.  beta < 1 or NaN is NSA_EBADARG; 2 is the
 * value of Barill et al. and the default of the Python layer.  A query with a non-finite coordinate gives NaN and counts 0; a mesh
 * without a usable face gives +0 (-0 with flip).
 *
 * What is bit-exact between implementations: the tree (keys, order, N, area, M, P, r2), every accept decision whose
 * |d2 - beta^2 r2| exceeds the rounding of both sides, and hence `accepted` and `evaluated`; w differs only through atan2, which is
 * not the same function in every maths library.  Worst cases, slow and never wrong: every face in one leaf (coincident centroids); a
 * query on the surface, which descends to the leaves about it.  A query far from the mesh accepts the root: one node.
 *
 * Workspace, a function of n_faces alone, every array rounded up to 256 bytes, with K(F) = the sum over l in [0, L(F)] of
 * min(8^l, F) (the most nodes a mesh of F faces can have; K(F) < 3.5 F for F >= 8):
 *   256 + 6 * 4 F + 4 + 100 K(F) + 2^18   bytes.
 * Nothing is allocated or synchronised; arguments are checked before the device is touched.  n_queries = 0 and n_faces = 0 return 0
 * without a launch (nothing is written).  The tree refers to the mesh by face number: the verts and faces given to
 * nsa_tri_winding_query are those given to nsa_tri_winding_build, unchanged. */

/* bytes of the tree buffer for n_faces (>= 1) faces; 0 for an invalid count */
uint64_t nsa_tri_winding_workspace(uint32_t n_faces);

/* Build the tree into `tree` (nsa_tri_winding_workspace(n_faces) bytes, device, 256-byte aligned).  info[3] (uint32, device; may be
 * NULL) receives L, the node count and the number of usable faces. */
int nsa_tri_winding_build(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, void *tree, uint32_t *info,
                          nsa_stream_t stream);

/* w[n_queries] float64.  accepted[n_queries] and evaluated[n_queries] uint32 (each may be NULL) receive the nodes used through their
 * dipole and the faces summed exactly -- measurements of the tree, not part of the answer. */
int nsa_tri_winding_query(const void *tree, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                          const float *queries, uint32_t n_queries, double beta, int flip, double *w, uint32_t *accepted,
                          uint32_t *evaluated, nsa_stream_t stream);

/* ---- Section 17: rays against a triangle mesh (csrc/mesh_raycast.hip) ---- */

/* Where does a ray o + t d hit the mesh: the smallest t in [tmin, tmax], the face and the barycentric coordinates of the hit -- or,
 * in any-hit mode, whether there is a hit at all.  Nothing in the reference casts rays against a mesh: this statement is the
 * contract, tests/raycast_ref.py restates it in numpy float64, and the kernels agree with that restatement BIT FOR BIT on t, the
 * face and the barycentrics; no tolerance is involved.  verts and faces as in Section 14; the tree is a buffer of its own.
 *
 * Inputs and arithmetic.  origins[n_rays][3] and dirs[n_rays][3] are fp32; a direction is not normalised, t is in units of |d|.
 * tmin and tmax are float64 (NaN: NSA_EBADARG; tmin > tmax: every ray misses).  The usable faces are exactly Section 14's.
 * Everything is float64 on the fp32 inputs, every operation rounded on its own (no FMA contraction); there is no transcendental
 * function anywhere, so +, -, *, / alone decide the bits.
 *
 * Face test (Woop, Benthin & Wald, "Watertight Ray/Triangle Intersection", JCGT 2013, in float64).  Per ray:
 *   kz = the index of the largest |d_k| (the lowest k on a tie) ; kx = kz + 1 mod 3 ; ky = kx + 1 mod 3 ; if d_kz < 0 swap kx, ky
 *   Sx = d_kx / d_kz ; Sy = d_ky / d_kz ; Sz = 1 / d_kz ; inv_k = 1 / d_k
 * Per face (a, b, c), with A = a - o, B = b - o, C = c - o:
 *   Ax = A_kx - Sx * A_kz ; Ay = A_ky - Sy * A_kz   (B, C alike)
 *   U = Cx * By - Cy * Bx ; V = Ax * Cy - Ay * Cx ; W = Bx * Ay - By * Ax
 *   miss if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0)
 *   det = (U + V) + W ; miss if det == 0
 *   NSA_RAY_CULL_BACK: miss if det < 0 (ab x ac points along d: the ray meets the face from behind) ; NSA_RAY_CULL_FRONT: if det > 0
 *   T = (U * (Sz * A_kz) + V * (Sz * B_kz)) + W * (Sz * C_kz) ; t = T / det ; barycentrics (U / det, V / det, W / det) for (a, b, c)
 *   miss unless enter <= t <= exit for the face's own box (below)
 * Two faces that share an edge with the same fp32 coordinates form that edge's function from the same products with the opposite
 * sign, exactly: no ray passes between them, and a ray through a shared edge or vertex hits at least one of the faces about it.
 *
 * Boxes.  A usable face has the fp32 box  s = the largest |coordinate| of its nine ; pad = fp32(s * 2^-20) ;
 *   lo_k = the next fp32 below fp32(min(a_k, b_k, c_k) - pad) ; hi_k = the next fp32 above fp32(max(a_k, b_k, c_k) + pad).
 * The slab interval of a ray against a box (lo, hi): per axis with d_k != 0, near_k and far_k = the min and max of
 * (lo_k - o_k) * inv_k and (hi_k - o_k) * inv_k; an axis with d_k == 0 passes iff lo_k <= o_k <= hi_k;
 *   enter = max(near_k, tmin) ; exit = min(far_k, tmax) ; the interval is empty when an axis fails or enter > exit.
 * The box clause is PART OF THE FACE TEST, and that is what makes pruning exact without an error analysis: a node's box is the fp32
 * min / max of the boxes below it, rounding is monotone, so a node's interval contains the interval of every face below it.  A node
 * with an empty interval cannot contain a hit; a node with enter > the best t so far cannot contain one that wins or ties.  The tree
 * and the brute force over all usable faces are equal by construction, in any traversal order.
 * The price: the pad must be wide enough that the clause never rejects what the edge functions accept.  The computed t places the hit
 * within about 2^-50 * D * (D / e) of the face, D = the distance of the face from o and e its shortest height (a ray grazing the
 * face's plane divides a small T by a small det); the pad is at least 2^-20 * s.  So the clause is idle while
 *   D^2 / e <= 2^30 * s,
 * which a mesh of 1 mm faces seen from a kilometre still meets.  tests/raycast_ref.py carries the test with and without the clause
 * and tests/test_mesh_raycast_cpu.py asserts that they agree on every ray of every case of the suite.
 *
 * Answer.  The hit with the smallest t, ties to the lowest face index: (t, face, barycentrics).  No hit: (+inf, -1, NaN).  A ray with
 * a non-finite component or d == 0: (NaN, -1, NaN), counts 0.  A mesh without a usable face: (+inf, -1, NaN).  A hit whose t
 * overflows to +inf is no hit.  NSA_RAY_ANY_HIT: the walk stops at the first hit it finds; face >= 0 iff some face is hit in
 * [tmin, tmax] -- that flag is the contract, t, face and the barycentrics are those of whichever hit was found.
 *
 * Tree.  Section 16's, rebuilt here into a buffer of its own: lo, side, L, the Morton key of each usable face's centroid, the stable
 * sort, a node for every level l in [0, L] and distinct prefix, numbered in pre-order.  Each node carries the box of its faces and,
 * per octant o = the 3 key bits of its level, the child of that octant.  No atomic takes part; two builds give identical bits.
 *
 * Walk of one ray, m = 4 * [d_x < 0] + 2 * [d_y < 0] + [d_z < 0], starting with visit(root):
 *   visit(i): n_nodes += 1 ; return if the node's interval is empty ; return if closest-hit and enter > best t
 *     at a leaf (level L): for each of its faces in sorted order: skip it if its own interval is empty, or if closest-hit and
 *        enter > best t ; else n_tested += 1 and the face test runs ; a hit replaces the best when t < best t, or t == best t and its
 *        face index is lower ; in any-hit mode the first hit ends the walk
 *     else: for r = 0 .. 7: visit(the child of octant r xor m) when the node has one
 * so the children nearer along the ray come first.  n_nodes and n_tested are functions of the inputs alone and the oracle
 * reproduces them exactly.  NSA_RAY_BRUTE tests every usable face in sorted order under the same skip rules (n_nodes = 0): the
 * on-device cross-check.  Worst cases, slow and never wrong: every centroid in one leaf; faces as large as the mesh.
 *
 * Workspace, a function of n_faces alone, every array rounded up to 256 bytes, K(F) as in Section 16:
 *   256 + 6 * 4 F + 4 + 24 F + 68 K(F) + 2^18   bytes.
 * Nothing is allocated or synchronised; arguments are checked before the device is touched.  n_rays = 0 and n_faces = 0 return 0
 * without a launch (nothing is written).  The verts and faces given to nsa_tri_ray_cast are those given to nsa_tri_ray_build. */

#define NSA_RAY_ANY_HIT 1u
#define NSA_RAY_CULL_BACK 2u
#define NSA_RAY_CULL_FRONT 4u
#define NSA_RAY_BRUTE 8u

/* bytes of the tree buffer for n_faces (>= 1) faces; 0 for an invalid count */
uint64_t nsa_tri_ray_workspace(uint32_t n_faces);

/* Build the tree into `tree` (nsa_tri_ray_workspace(n_faces) bytes, device, 256-byte aligned).  info[3] (uint32, device; may be NULL)
 * receives L, the node count and the number of usable faces. */
int nsa_tri_ray_build(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, void *tree, uint32_t *info,
                      nsa_stream_t stream);

/* t[n_rays] float64, face[n_rays] int32, bary[n_rays][3] float64 (may be NULL); n_nodes[n_rays] and n_tested[n_rays] uint32 (each may
 * be NULL) receive the nodes visited and the faces that went through the face test.  flags: a combination of NSA_RAY_*; both cull
 * bits at once, or an unknown bit, is NSA_EBADARG. */
int nsa_tri_ray_cast(const void *tree, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                     const float *origins, const float *dirs, uint32_t n_rays, double tmin, double tmax, uint32_t flags, double *t,
                     int32_t *face, double *bary, uint32_t *n_nodes, uint32_t *n_tested, nsa_stream_t stream);

/* ---- Section 18: mesh topology (edge table, watertightness, components joined across edges; DESIGN 4q, csrc/mesh_topology.hip) ---- */

/* The undirected edge table of faces[n_faces, 3] int32 over n_verts vertices, by index only, as in Section 11: coordinates play no
 * part and unwelded duplicates are different vertices.  n_verts < 2^31; H = 3 * n_faces < 2^31.  tests/topology_ref.py restates
 * this statement in numpy.  All of it is integer work: no floating point, no tolerance.
 *
 * Contributing faces.  A face CONTRIBUTES when its three indices lie in [0, n_verts), they are pairwise distinct, and face_mask
 * (uint8 [n_faces]; NULL = every face set) is non-zero for it.  F_c is their number, H_c = 3 F_c.  An index outside the range is
 * never dereferenced.  (Section 11's VALID face may be degenerate; here (a, a, b) does not contribute: it has no three edges.)
 *
 * Half-edges.  Half-edge h = 3 f + k (k = 0, 1, 2) of a contributing face f runs from faces[f][k] to faces[f][(k + 1) % 3].  Its EDGE
 * is the unordered pair (lo, hi), lo < hi, of the two; the half-edge is FORWARD when it runs lo -> hi.
 *
 * Edge table.  The E distinct edges are numbered in ascending (lo, hi) order, which is the ascending order of the 64-bit key
 * lo << 32 | hi.  Arrays sized by H, the first E entries valid (the rest are not written):
 *   edges[H, 2] int32         (lo, hi) of edge e
 *   edge_count[H] int32       the half-edges on it
 *   edge_forward[H] int32     how many of those are forward
 *   edge_start[H + 1] int32   CSR offsets into edge_halfedges: edge e owns [edge_start[e], edge_start[e + 1]); edge_start[E] = H_c
 * and
 *   edge_halfedges[H] int32   the half-edge ids sorted by edge, ascending id within an edge; the first H_c are valid, the rest -1
 *   face_edges[n_faces, 3]    int32: the edge id of half-edge 3 f + k; -1 (all three) for a face that does not contribute
 *
 * Classes.  edge_count == 1: BOUNDARY.  edge_count == 2: interior; it is INCONSISTENT when edge_forward != 1, that is, when its two
 * faces traverse it the same way.  edge_count > 2: NON-MANIFOLD; it is never counted as inconsistent.
 *
 * Boundary loops.  The connected components of the graph whose edges are the boundary edges, joined at shared vertices (so two
 * holes that touch in one vertex count once).  Computed with the vertex union-find of Section 11 (csrc/uf_passes.hpp), a boundary
 * edge uniting its two ends in place of a face uniting its three.
 *
 * totals[8] (uint64, device; the caller reads them once):
 *   {E, F_c, used vertices = distinct indices of contributing faces, boundary edges, non-manifold edges, inconsistent edges,
 *    boundary loops, status}
 * status: Section 11's bits (1: walk, 2: hook) from the boundary union-find; 0 unless the implementation is wrong.
 *
 * Kernel shape: the key sort is two stable argsorts of Section 4's radix sort, by hi and then by lo, each with only
 * the 8-bit passes n_verts needs; a half-edge that does not contribute carries n_verts in both and sorts last.  Run heads are found
 * by comparing neighbours in the sorted order, edge ids and forward counts by one exclusive scan of the head and forward flags, counts
 * as differences of run starts, and every total as a sum of per-block integer counts.  No atomics are used outside the union-find,
 * and those decide nothing in the output (parent[x] <= x): every output is a function of (faces, n_verts, face_mask) alone and
 * bit-reproducible.
 *
 * NULL faces, workspace, totals or output array, n_verts >= 2^31 or 3 * n_faces >= 2^31: NSA_EBADARG before anything is launched.
 * n_faces = 0 launches nothing, writes nothing and returns 0: all eight totals are zero by definition and the caller does not read
 * them.  n_verts = 0 with faces is legal (no face contributes).  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_faces = 0, 3 * n_faces >= 2^31, n_verts >= 2^31) */
uint64_t nsa_mesh_edges_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_edges(const int32_t *faces, uint32_t n_faces, uint32_t n_verts, const uint8_t *face_mask, void *workspace,
                   int32_t *edges, int32_t *edge_count, int32_t *edge_forward, int32_t *edge_start, int32_t *edge_halfedges,
                   int32_t *face_edges, uint64_t *totals, nsa_stream_t stream);

/* Face components, after nsa_mesh_edges on the same mesh, from its face_edges, edge_start and edge_halfedges.  Two contributing
 * faces are JOINED when they share an edge of any count >= 2; the closure is transitive.
 *   face_label[n_faces] int32   the smallest face index of the face's component, -1 for a face that does not contribute
 *   totals[2] (uint64, device)  {components, status}
 * A union-find over the faces with Section 11's uf_find / uf_unite unchanged: every half-edge of a run after the first unites its
 * face with its predecessor's.  The guarantees are Section 11's: parent[x] <= x, so the root is the smallest face index whatever the
 * interleaving and the atomics decide nothing in the output; step caps (n_faces steps) report through status (1: walk, 2: hook)
 * instead of spinning.  Input arrays that nsa_mesh_edges did not write give meaningless labels, never an access out of bounds.
 * Departure from trimesh: its face_adjacency pairs only edges with exactly two faces, so trimesh's split cuts a mesh at a
 * non-manifold edge; this rule joins across it.  (Python's face_adjacency keeps trimesh's definition.)
 * n_faces = 0 launches nothing and returns 0; NULL arguments or 3 * n_faces >= 2^31 are NSA_EBADARG before anything is launched. */

/* bytes of workspace; 0 for an invalid count (n_faces = 0 or 3 * n_faces >= 2^31) */
uint64_t nsa_mesh_face_components_workspace(uint32_t n_faces);

int nsa_mesh_face_components(const int32_t *face_edges, const int32_t *edge_start, const int32_t *edge_halfedges, uint32_t n_faces,
                             void *workspace, int32_t *face_label, uint64_t *totals, nsa_stream_t stream);

/* ---- Section 19: mesh simplification by vertex clustering with quadric placement (csrc/mesh_simplify.hip) ---- */

/* Rossignac-Borrel vertex clustering on a uniform grid, the representative of a cell placed by the error quadric of the faces around
 * it (Lindstrom's out-of-core form).  verts[n_verts, 3] fp32 and faces[n_faces, 3] int32 as in Section 14; optional normals and
 * colours fp32 [n_verts, 3]; origin[3] and h host float64 (finite, h > 0).  n_verts < 2^31, 3 * n_faces < 2^31.
 * tests/simplify_ref.py restates this statement in numpy float64.
 *
 * Arithmetic.  Float64 on the fp32 inputs, every operation rounded on its own (no FMA contraction), dot(u, w) and u x w in
 * Section 14's component order.  Everything after the cell of a vertex is integer work until the placement.
 *
 * Cells.  Vertex v has cell c_k = floor((double(v_k) - origin_k) / h) on axis k.  It is IN THE GRID when its three coordinates are
 * finite and 0 <= c_k < n_cells on every axis; n_cells <= 2^21, and the grid of the statement is n_cells = 2^21: a caller who knows
 * that every cell index is smaller may say so, which changes nothing but the number of sort passes (below).  Its key is
 * c_x * 2^42 + c_y * 2^21 + c_z.  The cell centre is origin + (c + 0.5) * h, computed as written.  (The quotient is rounded before
 * the floor, so a vertex within one float64 rounding of a cell face may be assigned across it: an output position lies in the
 * closed box of its cell up to a few float64 roundings of |v - origin| + h and the float32 rounding of the output.)
 *
 * Contributing faces.  A face CONTRIBUTES when its three indices lie in [0, n_verts) and all three vertices are in the grid.  The
 * indices need not be distinct (a repeated index gives a zero normal below and a face that cannot survive).  An index outside the
 * range is never dereferenced.  A vertex is USED when a contributing face names it.
 *
 * Clusters.  The K distinct keys of the used vertices, numbered 0 .. K - 1 in ascending key order.
 *   vertex_cluster[n_verts] int32    that number, -1 for a vertex that is not used
 *
 * Surviving faces.  A contributing face maps to its three cluster numbers.  It is COLLAPSED when they are not pairwise distinct.
 * Otherwise it is rotated cyclically until the smallest number comes first (the orientation is kept); among the faces with the
 * same rotated triple the one with the lowest face index SURVIVES, the others are DUPLICATES.  A triple and its reverse are
 * different faces and both stay: a sheet that collapses to zero thickness keeps its two sides.  The F' survivors are listed in
 * ascending original face index; the V' output vertices are the clusters a survivor names, in ascending cluster number.
 *   out_faces[n_faces, 3] int32      the first F' rows: the rotated triples, as indices of output vertices
 *   face_origin[n_faces] int32       the first F': the original face of each (strictly ascending)
 *   cluster_vertex[n_verts] int32    the first K: the output vertex of cluster k, -1 when no survivor names it; the rest -1
 *   out_cluster[n_verts] int32       the first V': the cluster of each output vertex (ascending)
 * totals[9] (uint64, device; the caller reads them once):
 *   {K, contributing faces, used vertices, vertices finite but outside the grid (used or not), collapsed faces, duplicate faces,
 *    V', F', status}
 * status: bit 1 when a sort order named an element outside its range; 0 unless the implementation is wrong (Section 18's style).
 *
 * Kernel shape.  Keys and used marks; the used vertices sorted by key with two stable argsorts of Section 4's radix
 * sort, low word then high word, a vertex that is not used carrying n_cells << 10 in the high word so that it sorts last, each
 * argsort with only the 8-bit passes the occupied width needs (low word: min(32, 21 + bits(n_cells - 1)) bits; high word:
 * bits(n_cells) + 10); run heads and an exclusive scan number the clusters.  The rotated triples are sorted by three chained
 * argsorts (third, second, first number; V for a face that cannot survive; passes by bits(n_verts)); a run head survives.  One scan
 * over the faces compacts them, one over the clusters numbers the output vertices.  Counts are sums of integers; every output is a
 * function of the arguments alone and bit-reproducible.
 *
 * NULL origin, non-finite origin, h non-finite or <= 0, n_cells = 0 or > 2^21, n_verts >= 2^31, 3 * n_faces >= 2^31, or (with both
 * counts non-zero) a NULL array, workspace or totals: NSA_EBADARG before anything is launched.  n_verts = 0 or n_faces = 0 launches
 * nothing, writes nothing and returns 0: all nine totals are zero and every vertex_cluster is -1 by definition, and the caller does
 * not read them.  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device), a function of the two counts alone; 0 for a count of 0 or out of range */
uint64_t nsa_mesh_cluster_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_cluster(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const double *origin, double h,
                     uint32_t n_cells, void *workspace, int32_t *vertex_cluster, int32_t *cluster_vertex, int32_t *out_cluster,
                     int32_t *out_faces, int32_t *face_origin, uint64_t *totals, nsa_stream_t stream);

/* Positions and attributes of the output vertices, after nsa_mesh_cluster on the same mesh, origin and h, from its vertex_cluster and
 * cluster_vertex.  n_out = V' (rows of the output arrays; an output vertex >= n_out is not written).  Per cluster that has an output
 * vertex, with coordinates relative to its own cell centre, p = double(v) - centre (component by component):
 *   m = (sum of p over its used vertices, in ascending vertex index) / count
 *   for every (contributing face f, corner j) whose corner vertex faces[f][j] is in the cluster, in ascending 3 f + j, with
 *   p0, p1, p2 the face's three vertices in the order listed, all relative to THIS cluster's centre:
 *     n = (p1 - p0) x (p2 - p0)        (not normalised: the weight is the squared area; no square root, no division)
 *     d = -dot(n, p0)
 *     A += n n^T  (A00 += n_x n_x, A01 += n_x n_y, A02 += n_x n_z, A11 += n_y n_y, A12 += n_y n_z, A22 += n_z n_z) ;  b += n * d
 *   tr = (A00 + A11) + A22
 *   placement 0 (mean):     x = m
 *   placement 1 (quadric):  x = m when tr == 0; otherwise mu = eps * tr, r = -b + mu * m, (A + mu I) s = r solved by Cholesky
 *                           (L L^T, no pivoting: the matrix is symmetric positive definite for eps > 0, condition <= ~1 / eps),
 *                           x_k = s_k clamped to [-h / 2, h / 2]; x = m when a component of s is not finite (possible with eps = 0 only)
 *   position = float(centre + x)
 * This is Lindstrom's quadric with a Tikhonov pull towards the cluster mean in place of his truncated SVD: no threshold and no
 * branch on a singular value; the rule is continuous in its inputs, the clamp included.
 *   out_normals  = (sum of the used member vertices' normals, ascending vertex index) / its Euclidean length
 *                  sqrt((x * x + y * y) + z * z); (0, 0, 0) when that length is zero or not finite
 *   out_colours  = (sum of the member colours, same order) / count
 *   out_cell[n_out, 3] int32 (may be NULL)   the cell of each output vertex
 * normals and out_normals are both NULL or both given, likewise colours and out_colours.
 *
 * Kernel shape.  The vertices sorted stably by cluster and the incidences 3 f + j sorted stably by the cluster of the corner vertex
 * (one argsort each, passes by bits(n_verts)), so every cluster owns a run in the stated order; one lane per output vertex walks
 * its two runs.  No atomics: each sum has the one order above, and two runs are bit-identical.  Input arrays that nsa_mesh_cluster
 * did not write give meaningless positions, never an access out of bounds.
 *
 * eps < 0 or not finite, placement not 0 or 1, n_out > n_verts, an attribute without its output or the reverse, the grid errors of
 * nsa_mesh_cluster, or (with all three counts non-zero) a NULL verts, faces, vertex_cluster, cluster_vertex, workspace or out_verts:
 * NSA_EBADARG before anything is launched.  A count of zero launches nothing and returns 0.  Nothing is allocated or synchronised. */

/* bytes of workspace, a function of the two counts alone; 0 for a count of 0 or out of range */
uint64_t nsa_mesh_cluster_place_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_cluster_place(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const float *normals,
                           const float *colours, const double *origin, double h, double eps, int placement,
                           const int32_t *vertex_cluster, const int32_t *cluster_vertex, uint32_t n_out, void *workspace,
                           float *out_verts, float *out_normals, float *out_colours, int32_t *out_cell, nsa_stream_t stream);

/* ---- Section 20: mesh orientation (consistent winding, orientability, outward by volume; DESIGN 4s, csrc/mesh_orient.hip) ---- */

/* A consistent winding for faces[n_faces, 3] int32, after nsa_mesh_edges (Section 18) on the same mesh, from its face_edges,
 * edge_start, edge_halfedges and its totals as they lie on the device (totals[0] = E is read there, never on the host).
 * 3 * n_faces < 2^31.  tests/orient_ref.py restates this statement as a sequential breadth-first two-colouring.  Integer work only.
 *
 * Joining rule.  Two contributing faces are JOINED across an edge only when that edge carries exactly two half-edges (trimesh's
 * face_adjacency rule).  An edge with one half-edge, or with three or more, joins nothing: a winding across a non-manifold edge
 * is not defined.  Half-edge 3 f + k runs faces[f][k] -> faces[f][(k + 1) % 3]; the two faces AGREE when their half-edges run in
 * opposite directions along the edge.  The closure is transitive.  (Departure from Section 18's face components, which join across
 * every edge of count >= 2: orient_label cuts at a non-manifold edge, as trimesh's split does.)
 *
 * Double cover.  2 * n_faces nodes: node 2 f is face f as given, node 2 f + 1 is face f reversed.  An agreeing pair (f, g)
 * unites 2 f ~ 2 g and 2 f + 1 ~ 2 g + 1; a disagreeing pair unites 2 f ~ 2 g + 1 and 2 f + 1 ~ 2 g.  The union-find is Section
 * 11's uf_find / uf_unite, unchanged.  After all unions, with r0 = find(2 f) and r1 = find(2 f + 1):
 *   orient_label[n_faces] int32   min(r0, r1) >> 1: the smallest face index of the face's component; -1 for a face that does not
 *                                 contribute
 *   orientable[n_faces] uint8     r0 != r1.  A component whose two sheets meet is not orientable (a Moebius strip, a Klein bottle);
 *                                 the value is the same for every face of a component; 0 for a face that does not contribute
 *   flip[n_faces] uint8           orientable and r0 > r1.  Reversing the flipped faces winds every orientable component consistently
 *                                 with its smallest face, which keeps its winding; a non-orientable component is left as it is
 * totals[4] (uint64, device): {components, non-orientable components, flipped faces, status}
 * status: Section 11's bits (1: walk, 2: hook); 0 unless the implementation is wrong.
 *
 * Determinism.  parent[x] <= x holds throughout, so a root is the smallest node of its tree whatever the interleaving, and the
 * atomics decide nothing in the output: every output is a function of the arguments alone and bit-reproducible.  Input arrays that
 * nsa_mesh_edges did not write give meaningless outputs, never an access out of bounds.
 *
 * Kernel shape: one lane per edge for the unions, one per face for the labels, per-block integer counts added by one
 * workgroup.  No floating point, no atomics outside the union-find (and the or of its cap report).
 *
 * NULL arguments or 3 * n_faces >= 2^31: NSA_EBADARG before anything is launched.  n_faces = 0 launches nothing, writes nothing and
 * returns 0.  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_faces = 0 or 3 * n_faces >= 2^31) */
uint64_t nsa_mesh_orient_workspace(uint32_t n_faces);

int nsa_mesh_orient(const int32_t *faces, uint32_t n_faces, const int32_t *face_edges, const int32_t *edge_start,
                    const int32_t *edge_halfedges, const uint64_t *edge_totals, void *workspace, int32_t *orient_label,
                    uint8_t *orientable, uint8_t *flip, uint64_t *totals, nsa_stream_t stream);

/* Outward by volume, after nsa_mesh_orient on the same mesh: which of its two consistent windings an orientable, closed component
 * gets.  verts[n_verts, 3] fp32; origin[3] fp32 ON THE DEVICE (the caller passes o = the centre of the bounding box of the used
 * vertices rounded to fp32; any finite point gives a valid rule, a point near the mesh the tightest bound).
 * tests/orient_ref.py restates this with math.fsum.
 *
 * Components are those of orient_label.  A component is CLOSED when every half-edge of its faces lies on an edge of count 2
 * (edge_start[e + 1] - edge_start[e] == 2).  The rule is strict: a tetrahedron that touches another along an edge is not closed.
 * Per component c of n_c faces, in float64 on the fp32 inputs, every operation rounded on its own:
 *   S_c = (sum over its faces of s_f * det(a - o, b - o, c - o)) / 6,   s_f = -1 for a flipped face, +1 otherwise
 *   P_c = (sum over its faces of perm(|a - o|, |b - o|, |c - o|)) / 6   (the same six products with absolute values)
 *   det(a, b, c) = (a_x (b_y c_z - b_z c_y) + a_y (b_z c_x - b_x c_z)) + a_z (b_x c_y - b_y c_x)
 * The component is DECIDED when it is closed, orientable and |S_c| > (n_c + 16) * 2^-52 * P_c, the forward error bound of the sum,
 * doubled; a decided component is TOGGLED when S_c < 0.  Open, non-orientable and undecided components keep nsa_mesh_orient's
 * winding.  The sums are indexed by the component's label (its smallest face); entries at other indices are not written:
 *   comp_S[n_faces], comp_P[n_faces] float64;  comp_n[n_faces] int32;  comp_flags[n_faces] uint8: 1 closed | 2 decided | 4 toggled
 *   flip_out[n_faces] uint8     flip[f] xor toggled(component of f); 0 for a face that does not contribute
 * totals[5] (uint64, device): {closed components, decided components, toggled components, flipped faces after the toggles, status}
 * status: 4 when the sort order is not a permutation or a run does not start at its label; 0 unless the implementation is wrong.
 *
 * Order of the additions.  The faces are sorted stably by label (Section 4's radix argsort), so a component is one run in ascending
 * face index.  Blocks of 1024 sorted positions: within a block a segmented Hillis-Steele scan (x_t += x_(t - d), d = 1, 2, 4, ...,
 * while t - d is in the same run and block); a run that crosses blocks leaves one partial per block, and those are added by 256
 * threads, thread t taking partials t, t + 256, ... in order, then a binary tree over the threads.  No atomics: the sums are a
 * function of the arguments alone and bit-reproducible; they are NOT the sums in face order (the bound above covers any order).
 *
 * NULL arguments (verts may be NULL when n_verts = 0), n_verts >= 2^31 or 3 * n_faces >= 2^31: NSA_EBADARG before anything is
 * launched.  n_faces = 0 launches nothing and returns 0.  A face index outside [0, n_verts) is never dereferenced (the face adds
 * zero).  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_faces = 0 or 3 * n_faces >= 2^31) */
uint64_t nsa_mesh_orient_volume_workspace(uint32_t n_faces);

int nsa_mesh_orient_volume(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, const int32_t *face_edges,
                           const int32_t *edge_start, const int32_t *orient_label, const uint8_t *orientable, const uint8_t *flip,
                           const float *origin, void *workspace, double *comp_S, double *comp_P, int32_t *comp_n,
                           uint8_t *comp_flags, uint8_t *flip_out, uint64_t *totals, nsa_stream_t stream);

/* ---- Section 21: mesh smoothing (vertex rings, Laplacian / Taubin steps, vertex normals; DESIGN 4t, csrc/mesh_smooth.hip) ---- */

/* The vertex rings of a mesh, after nsa_mesh_edges (Section 18) on the same mesh, from its edges and its totals as they lie on the
 * device (totals[0] = E is read there, never on the host).  6 * n_faces < 2^31 (the offsets are int32), n_verts < 2^31.
 * tests/smooth_ref.py restates this section in numpy.  Integer work only; no atomics.
 *   ring_start[n_verts + 1] int32   CSR offsets: row v owns [ring_start[v], ring_start[v + 1]); ring_start[n_verts] = 2 E
 *   ring[6 * n_faces] int32         the neighbour index;          the first 2 E entries are valid, the rest are not written
 *   ring_edge[6 * n_faces] int32    the edge id of {v, neighbour}, so any per-edge property (edge_count) is one gather
 * Row v lists every u with {u, v} an edge, in ascending u: the neighbours below v come from the edges with hi == v, those above from
 * the edges with lo == v.  A vertex on no contributing face has an empty row.
 *
 * Kernel shape: the edge table is sorted by (lo, hi); one stable argsort of Section 4's radix sort by hi, with only the
 * 8-bit passes n_verts needs, gives the (hi, lo) order (the 3 * n_faces - E positions past E carry n_verts and sort last).  Then
 * ring_start[v] = #{lo < v} + #{hi < v}, two binary searches and no scan, and the slot of every entry is a closed form of the two
 * counts.  Every output is a function of the arguments alone and bit-reproducible.  An edge with an end outside [0, n_verts) takes no
 * part; arrays that nsa_mesh_edges did not write give meaningless rows, never an access out of bounds.
 *
 * NULL arguments, n_verts >= 2^31 or 6 * n_faces >= 2^31: NSA_EBADARG before anything is launched.  n_faces = 0 launches nothing,
 * writes nothing and returns 0 (every row is empty by definition).  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_faces = 0, 6 * n_faces >= 2^31, n_verts >= 2^31) */
uint64_t nsa_mesh_ring_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_ring(const int32_t *edges, const uint64_t *edge_totals, uint32_t n_verts, uint32_t n_faces, void *workspace,
                  int32_t *ring_start, int32_t *ring, int32_t *ring_edge, nsa_stream_t stream);

#define NSA_SMOOTH_FREE 0   /* boundary vertices move like any other */
#define NSA_SMOOTH_FIXED 1  /* boundary vertices keep their input */
#define NSA_SMOOTH_CURVE 2  /* a boundary vertex is smoothed along the boundary edges only */

/* n_steps smoothing steps over the rings of nsa_mesh_ring, with the edge_count of nsa_mesh_edges for the same mesh.  verts[n_verts, 3]
 * fp32; fixed[n_verts] uint8 or NULL; factors[n_steps] float64 ON THE HOST, |f| <= 1 (Laplacian: lambda repeated; Taubin: lambda,
 * mu, lambda, mu, ...); boundary one of NSA_SMOOTH_*; max_move > 0, +inf for none.  All float64 on the fp32 inputs, every operation
 * rounded on its own, nothing contracted; tests/smooth_ref.py restates it operation by operation and the device equals it bit for bit.
 *
 * x^0_v = double(verts[v]).
 *   live(v)          the row of v is not empty and its three coordinates are finite
 *   on_boundary(v)   some entry of its row lies on an edge with edge_count == 1
 *   v MOVES          live(v), fixed[v] == 0, and not (boundary == FIXED and on_boundary(v))
 *   N'(v)            the entries u of the row with live(u), in row order; when boundary == CURVE and on_boundary(v) only those whose
 *                    edge has edge_count == 1, so a rim is smoothed along itself and does not creep inward.  A non-manifold edge is
 *                    an ordinary edge.
 * One step with factor f, for all vertices at once from the previous step's positions: a moving v with n = |N'(v)| > 0 gets, per
 * component,  s = ((x_u1 + x_u2) + x_u3) + ...,  m = s / n,  d = m - x_v,  y_v = x_v + f * d,  and with a finite max_move
 * y_v = min(max(y_v, x^0_v - max_move), x^0_v + max_move).  Every other vertex keeps x_v.
 * out[n_verts, 3] fp32: the positions after the last step rounded to nearest.  A vertex that cannot move -- not live, fixed, held at
 * the boundary, or without a live neighbour -- is returned with its input BITS, NaN payloads included.  n_steps = 0 copies the input.
 * state[n_verts] uint8 (out): 1 live | 2 on_boundary | 4 moves | 8 moves and |N'| > 0.
 *
 * Kernel shape: a prologue writes the float64 positions and the state byte, a second pass compacts every row to N' (both
 * are constant over the steps), then one launch per step, one lane per vertex, over ping-pong float64 positions in the workspace; the
 * last step rounds to fp32.  No atomics anywhere.
 *
 * NULL arguments (fixed may be NULL; the ring arrays and edge_count may be NULL when n_faces = 0, factors when n_steps = 0), a factor
 * with |f| > 1 or NaN, max_move <= 0 or NaN, an unknown boundary, n_verts >= 2^31 or 6 * n_faces >= 2^31: NSA_EBADARG before anything
 * is launched.  n_verts = 0 launches nothing and returns 0.  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_verts = 0 or >= 2^31, 6 * n_faces >= 2^31) */
uint64_t nsa_mesh_smooth_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_smooth(const float *verts, uint32_t n_verts, uint32_t n_faces, const int32_t *ring_start, const int32_t *ring,
                    const int32_t *ring_edge, const int32_t *edge_count, const uint8_t *fixed, const double *factors, uint32_t n_steps,
                    int boundary, double max_move, void *workspace, float *out, uint8_t *state, nsa_stream_t stream);

#define NSA_NORMALS_AREA 0
#define NSA_NORMALS_ANGLE 1

/* Vertex normals from the faces.  verts[n_verts, 3] fp32, faces[n_faces, 3] int32, 3 * n_faces < 2^31; weighting one of NSA_NORMALS_*.
 * The CORNERS are c = 3 f + k of the faces that contribute by Section 18's rule (indices in [0, n_verts), pairwise distinct) and whose
 * three vertices are finite.  At corner c, with p0 the corner's vertex, p1 the next and p2 the previous vertex of the face, in float64
 * from the fp32 coordinates, every operation rounded on its own:
 *   a = p1 - p0,  b = p2 - p0,  n = a x b = (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x)
 * which follows the face winding (mesh_eval's face normal).  Per vertex, over its corners in ASCENDING c, starting from zero:
 *   AREA:   N = sum of n
 *   ANGLE:  N = sum of theta * (n / |n|),  |n| = sqrt((n_x^2 + n_y^2) + n_z^2),  theta = atan2(|n|, (a_x b_x + a_y b_y) + a_z b_z);
 *           corners with |n| = 0 are skipped
 * normals[n_verts, 3] fp32 = N / |N| rounded to nearest, |N| = sqrt((N_x^2 + N_y^2) + N_z^2); the zero vector when |N| is zero or not
 * finite, which covers a vertex without a corner.  The AREA form is + - * / and sqrt only and equals tests/smooth_ref.py bit for bit;
 * the ANGLE form depends on the device's atan2 in the last bits of float64.
 * The corner-by-vertex order is one stable argsort of the 3 F corner keys (csrc/corner_table.hpp, shared with Section 15's
 * adjacency).  No atomics; bit-reproducible.
 *
 * NULL arguments (faces and workspace may be NULL when n_faces = 0), an unknown weighting, n_verts >= 2^31 or 3 * n_faces >= 2^31:
 * NSA_EBADARG before anything is launched.  n_verts = 0 launches nothing.  Nothing is allocated or synchronised. */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (a zero count, n_verts >= 2^31, 3 * n_faces >= 2^31) */
uint64_t nsa_mesh_vertex_normals_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_vertex_normals(const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces, int weighting, void *workspace,
                            float *normals, nsa_stream_t stream);

/* ---- Section 22: mesh decimation (parallel edge collapse with quadric error; DESIGN 4u, csrc/mesh_decimate.hip) ---- */

/* Garland-Heckbert edge collapse in ROUNDS of independent collapses.  The caller drives the rounds: per round nsa_mesh_edges (Section
 * 18) and nsa_mesh_ring (Section 21) on the CURRENT faces, then nsa_mesh_decimate_round, then one read of totals.  verts[n_verts, 3]
 * fp32, faces[n_faces, 3] int32 (the caller's working copy, rewritten in place), 6 * n_faces < 2^31, n_verts < 2^31.
 * tests/decimate_ref.py restates this section in numpy and the device equals it element for element, bit for bit.
 *
 * Arithmetic.  Float64 throughout, + - * / only, every operation rounded on its own (nothing contracted), every sum in the stated
 * order; (u . w) = (u_x w_x + u_y w_y) + u_z w_z; u x w = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x).  No square root
 * and no transcendental function: a cost that differs in its last bit changes which edge wins.  No atomics anywhere.
 *
 * State (nsa_mesh_decimate_state_bytes, device, the caller's, opaque): per vertex x_v = double(verts[v]); the quadric
 * Q_v = (a00, a01, a02, a11, a12, a22, b0, b1, b2, c, w), eleven float64; the colour double(colors[v]) when colors is given;
 * vertex_map[v] = v; the bytes locked(v) and moved(v) = 0; and the number of log rows written.
 *
 * nsa_mesh_decimate_init, from the edge table and the rings of the input faces:
 *   plane(n, p, s): d = -(n . p); adds s n_i n_j to a_ij as (s n_i) n_j, (s n_i) d to b_i, (s d) d to c and s (n . n) to w; without
 *   a scale the products are n_i n_j, n_i d, d d and n . n.
 *   A face is FINITE when it contributes by Section 18's rule and its nine coordinates are finite; its n = (p1 - p0) x (p2 - p0),
 *   unnormalised, p_k the vertex at faces[f][k].
 *   Q_v, starting from zero: first plane(n, p0) of every finite face at v, in ascending corner id 3 f + k (csrc/corner_table.hpp, one
 *   lane per vertex); then, along the row of v in ascending neighbour u, for every edge {u, v} with edge_count == 1 whose face is
 *   finite: e = x_hi - x_lo, m = e x n, s = boundary_weight / (e . e), plane(m, x_lo, s), skipped when e . e is not positive or s
 *   is not finite.  (Garland and Heckbert's boundary constraint; m . m = (e . e)(n . n), so the weight is boundary_weight n . n in
 *   the units of the face terms.)
 *   locked(v): a coordinate of v is not finite; fixed[v] != 0; or some entry u of its row is not finite (v is then a vertex of a face
 *   with a non-finite vertex), lies on an edge with edge_count > 2, or -- boundary == NSA_DECIMATE_BOUNDARY_FIXED -- on an edge with
 *   edge_count == 1.  A locked vertex never takes part in a collapse; the locks are those of the input and do not change.
 *
 * nsa_mesh_decimate_round, for every edge i = (lo, hi) of the current table, the first failing test giving its class:
 *   LOCK     locked(lo) or locked(hi), or edge_count not 1 or 2.
 *   Placement.  Q = Q_lo + Q_hi (component by component), m = (x_lo + x_hi) * 0.5, tr = (a00 + a11) + a22, mu = eps * tr.  With
 *            A' = A + mu I on the diagonal and r = mu * m - b, LDL^T in the pivot order 0, 1, 2:
 *              d0 = a'00; l10 = a01 / d0; l20 = a02 / d0; d1 = a'11 - l10 a01; t = a12 - l20 a01; l21 = t / d1;
 *              d2 = (a'22 - l20 a02) - l21 t;  y0 = r0; y1 = r1 - l10 y0; y2 = (r2 - l20 y0) - l21 y1;
 *              x2 = y2 / d2; x1 = y1 / d1 - l21 x2; x0 = (y0 / d0 - l10 x1) - l20 x2.
 *            x = m when tr is zero or not finite, a pivot d0, d1, d2 is not positive, or x is not finite.
 *   Cost.    (A x)_i = (a_i0 x0 + a_i1 x1) + a_i2 x2; cost = ((x . A x) + 2 (b . x)) + c with the un-regularised Q, then max(0, cost).
 *   ERROR    the cost is not finite, or has_limit and not cost <= max_error2 * w (max_error2 = max_error^2, squared by the caller:
 *            the n . n weighted mean squared distance to the planes collected so far).
 *   LINK     common = the size of the intersection of the two ascending rows; virt = 1 when edge_count == 2 and both ends have a row
 *            entry on an edge with edge_count == 1 (both touch the virtual vertex beyond the boundary), else 0; fails unless
 *            common + virt == edge_count, and unless |row lo| + |row hi| - common (the union, both ends included) >= 5, or >= 4 for
 *            edge_count == 1: the merged vertex keeps three neighbours, two along a boundary.
 *   FOLD     every face around lo or hi that does not hold both, with n before and n' with that end at x: fails unless
 *            (n . n') > 0 and (n . n')^2 > (min_cos2 * (n . n)) * (n' . n').  A zero n or n' fails.
 *   CANDIDATE otherwise; its KEY is (the uint64 bits of cost, mix(lo << 32 | hi)).  Non-negative doubles order as their bits.  mix is
 *            the finaliser of splitmix64 on 64-bit words -- z = w + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *            z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31) -- a bijection, so every key is distinct.  (The plain word
 *            lo << 32 | hi would do for that, but it orders equal costs by the vertex numbering: on a flat region, where every cost
 *            is exactly 0, a lattice numbered row by row then has two or three local minima and a round takes as many collapses.)
 * Selection: m1(v) = the smallest key over the candidate edges of row v; m2(v) = the smallest m1 over v and its row; an edge is
 * SELECTED iff its key equals m2(lo) and m2(hi).  No end of a selected edge lies within one edge of an end of another,
 * so the round equals its collapses applied one after another in any order, and the globally smallest candidate is always selected.
 * Prefix: the selected edges in ascending key (four stable radix argsorts, the two halves of the edge word and then of the cost
 * bits, least significant first); with has_target the edge at sorted position p is TAKEN iff F_c - (the sum of edge_count over the positions
 * before p) > target_faces, F_c the contributing faces of the table; without, all are taken.  A collapse removes edge_count faces.
 * Application, per taken edge: with colours t = ((x - x_lo) . e) / (e . e), e = x_hi - x_lo (0 when e . e is not positive), clamped
 * to [0, 1], colour_lo += t * (colour_hi - colour_lo); x_lo = x; Q_lo = Q; vertex_map[hi] = lo; moved(lo) = 1; the row
 * (round, lo, hi, cost bits) goes to log[4 * (rows so far + p)] when that row is below log_rows.  Then every corner naming hi names
 * lo (a collapsed face has a repeated index and stops contributing by Section 18's rule: nothing is compacted), and vertex_map is
 * composed so that every entry names a vertex that maps to itself.
 * totals[14] (uint64, device): {round, E, F_c before, candidates, rejected by lock, by error, by link, by fold, selected, taken,
 *   faces removed, F_c after, log rows so far, status (1: a sort order left its range; 0 unless the implementation is wrong)}.
 *
 * nsa_mesh_decimate_finish: out_verts = the input BITS of a vertex that never moved, else x_v rounded to fp32; out_colors likewise;
 * vertex_map[v] = the surviving vertex v was merged into.
 *
 * Kernel shape: one lane per edge slot, vertex or corner; the totals and the prefix rule in one workgroup.  Every index
 * read from a table is range-checked before use, and every loop runs over a row or run whose ends were checked against the table's
 * length.  NULL arguments (colors, fixed and -- with log_rows = 0 -- log may be NULL), an unknown boundary, a negative or non-finite
 * boundary_weight or eps, min_cos2 outside [0, 1), a negative max_error2 with has_limit, n_verts >= 2^31 or 6 * n_faces >= 2^31:
 * NSA_EBADARG before anything is launched.  n_verts = 0 or n_faces = 0 launches nothing and returns 0.  Nothing is allocated or
 * synchronised. */

#define NSA_DECIMATE_BOUNDARY_QUADRIC 0  /* boundary edges add their constraint planes */
#define NSA_DECIMATE_BOUNDARY_FIXED 1    /* and their ends are locked */

/* bytes of the state (256-byte aligned, device); 0 for n_verts = 0 or >= 2^31 */
uint64_t nsa_mesh_decimate_state_bytes(uint32_t n_verts);

/* bytes of workspace for init and round (256-byte aligned, device); 0 for an invalid count (a zero count, n_verts >= 2^31,
 * 6 * n_faces >= 2^31) */
uint64_t nsa_mesh_decimate_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_decimate_init(const float *verts, const float *colors, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                           const int32_t *edge_count, const int32_t *edge_start, const int32_t *edge_halfedges, const int32_t *ring_start,
                           const int32_t *ring, const int32_t *ring_edge, const uint8_t *fixed, int boundary, double boundary_weight,
                           void *workspace, void *state, nsa_stream_t stream);

int nsa_mesh_decimate_round(uint32_t n_verts, int32_t *faces, uint32_t n_faces, const int32_t *edges, const int32_t *edge_count,
                            const int32_t *edge_start, const int32_t *edge_halfedges, const uint64_t *edge_totals,
                            const int32_t *ring_start, const int32_t *ring, const int32_t *ring_edge, uint32_t round, int has_target,
                            uint64_t target_faces, int has_limit, double max_error2, double min_cos2, double eps, int has_colors,
                            void *workspace, void *state, uint64_t *log, uint32_t log_rows, uint64_t *totals, nsa_stream_t stream);

int nsa_mesh_decimate_finish(const float *verts, const float *colors, uint32_t n_verts, const void *state, float *out_verts,
                             float *out_colors, int32_t *vertex_map, nsa_stream_t stream);

/* ---- Section 23: hole filling (boundary loops traced, ranked and patched; DESIGN 4v, csrc/mesh_fill.hip) ---- */

/* Closes the holes of a mesh with polar patches, after nsa_mesh_edges (Section 18) on the same face list.  verts[n_verts, 3] fp32,
 * optional colors fp32 [n_verts, 3], faces[n_faces, 3] int32, n_verts < 2^31, H = 3 * n_faces < 2^31.  names (NULL = faces) is the
 * face list the edge table was built from when that is not faces itself (welded names, mesh_eval.welded_faces); the topology and the
 * pinch test read names, the positions and the patch read faces.  n_boundary = B is the number of boundary edges in the edge table's
 * totals, which the caller has read back.  tests/fill_ref.py restates this section in numpy and the device equals it element for
 * element, bit for bit.
 *
 * Arithmetic.  Float64 throughout on the fp32 inputs, + - * / only, every operation rounded on its own (nothing contracted), every
 * sum in the stated order starting from zero; (u . w) = (u_x w_x + u_y w_y) + u_z w_z; u x w = (u_y w_z - u_z w_y, u_z w_x - u_x w_z,
 * u_x w_y - u_y w_x).  No square root and no transcendental function.  No atomics anywhere.
 *
 * Items.  A BOUNDARY half-edge h = 3 f + k runs a -> b on an edge with edge_count == 1 (Section 18's half-edges and classes).  The B
 * boundary half-edges in ascending id are the ITEMS 0 .. B - 1 (one exclusive scan of the flags).
 *
 * Successor.  From g = 3 f + (k + 1) % 3, which leaves b: while the edge of g is not a boundary edge -- it must have edge_count == 2
 * and edge_forward == 1, otherwise the item is BLOCKED -- step to the twin t, the other entry of the edge's run in edge_halfedges,
 * and set g = 3 (t / 3) + (t % 3 + 1) % 3, which leaves b again.  More than n_faces steps set status bit 1 and block the item.
 * next(i) = the item of g; a blocked item is its own successor and a TERMINAL.  Rotation stays inside one fan of faces.
 *
 * Pinch.  An item is PINCHED when another item starts at the same vertex (by name): one stable radix argsort of the B start
 * vertices (Section 4's sort) and a comparison with the two neighbours in that order.
 *
 * Loops.  ceil(log2(max(B, 2))) + 1 double-buffered rounds of pointer jumping, each item carrying (smallest item seen, jump pointer,
 * reached a terminal).  An item that reaches a terminal lies on an OPEN CHAIN and belongs to no loop.  Otherwise its LEADER is the
 * smallest item of its cycle.  As many rounds of Wyllie's list ranking, the cycle cut in front of its leader, give rank(i), the
 * steps from the leader, and the loop's length n.  The L loops are numbered in ascending leader; loop_start is the exclusive scan
 * of n over the leaders; order[loop_start + rank] = h.  (Departure from Section 18, which counts the components of the boundary
 * graph: the counts agree when no item is pinched or blocked.  Two holes that touch in a vertex are one component there and one
 * figure-eight loop here, the rotation running from one hole into the other through the fan between them; it holds two pinched
 * items and is not filled.  A boundary that runs into a non-manifold or inconsistent edge is an open chain.)
 *
 * Per loop, one lane walking its segment of order in rank order, p_i the start vertex of its i-th half-edge, i + 1 taken mod n:
 *   c = (sum p_i) / n;  the mean colour likewise when colors is given (zero otherwise)
 *   box lo / hi: a running "if p < lo: lo = p" / "if p > hi: hi = p" from p_0;  D2 = |hi - lo|^2
 *   R2 = (sum |p_i - c|^2) / n;  L2 = (sum |p_{i+1} - p_i|^2) / n
 *   n_i = (p_{i+1} - c) x (p_i - c);  A = sum n_i
 * Class, the first that applies: NONFINITE 1 (a coordinate of some p_i is not finite; the row's reals are zero and its ring count
 * 0), PINCHED 2 (it holds a pinched item), TOO_MANY_EDGES 3 (has_max_edges and n > max_edges), TOO_LARGE 4 (has_max_size and
 * D2 > max_size2, squared by the caller), FOLDED 5 (skip_folded and some n_i . A <= 0: the loop is not star-shaped about c),
 * FILLED 0.  Ring count K = rings when rings > 0; else the smallest K >= 1 with (double(K) * double(K)) * L2 >= R2, at most max_rings.
 * A filled loop gets new_verts = (K - 1) n + 1 and new_faces = n (2 K - 1), every other loop 0 and 0; vert_offset and face_offset
 * are their exclusive scans over the loops.
 *   loop_ints[B, 9] int64, the first L rows: leader half-edge, n, loop_start, class, K, new_verts, new_faces, vert_offset, face_offset
 *   loop_reals[B, 18] float64, the first L rows: c, mean colour, box lo, box hi, D2, R2, L2, A
 *   halfedges[B], next[B] (items), leader[B] (item, -1 on an open chain), rank[B] int32; flags[B] uint8: 1 blocked | 2 pinched |
 *   4 open chain | 8 the step cap was hit; order[B] int32, the first B - (open-chain items) valid
 *   totals[12] (uint64, device): {B, L, filled, nonfinite, pinched, too_many_edges, too_large, folded, open-chain items,
 *   new vertices, new faces, status (1: a rotation hit its cap; 2: the flags do not add up to n_boundary; 0 unless the input arrays
 *   are not Section 18's of this face list)}
 *
 * nsa_mesh_fill_emit, after one read of totals[9] and totals[10].  Ring 0 of a filled loop is the loop itself, r_0[i] the start
 * vertex of order[loop_start + i]; ring j, 1 <= j < K, is q_{j,i} = c + t_j * (p_i - c), t_j = double(K - j) / double(K), at index
 * n_verts + vert_offset + (j - 1) n + i; the centre c at n_verts + vert_offset + (K - 1) n.  Colours by the same formula about the
 * mean colour.  Positions and colours are rounded to fp32.  Faces run against the boundary half-edges: between rings j and j + 1
 * (r_j[i+1], r_j[i], r_{j+1}[i]) then (r_j[i+1], r_{j+1}[i], r_{j+1}[i+1]); from the last ring (r_{K-1}[i+1], r_{K-1}[i], centre).
 * Face order is by loop, then ring, then i.  new_verts[n_new_verts, 3], new_colors and new_faces[n_new_faces, 3] hold the appended
 * rows alone: the caller keeps the old vertices and faces in front of them, bit for bit.
 *
 * Kernel shape: one lane per half-edge, item or loop; one lane per new face in emit, the first face of (ring, i) writing
 * the vertex there.  Every index read from a table is range-checked before use.  NULL arguments (colors / new_colors together, names),
 * rings or max_rings > 65535, max_rings = 0, a negative or NaN max_size2 with has_max_size, n_boundary > 3 * n_faces,
 * n_verts + n_new_verts >= 2^31, n_verts >= 2^31 or 3 * n_faces >= 2^31: NSA_EBADARG before anything is launched.  n_faces = 0 or
 * n_boundary = 0 (and n_new_faces = 0 in emit) launches nothing, writes nothing and returns 0.  Nothing is allocated or synchronised. */

#define NSA_FILL_FILLED 0
#define NSA_FILL_NONFINITE 1
#define NSA_FILL_PINCHED 2
#define NSA_FILL_TOO_MANY_EDGES 3
#define NSA_FILL_TOO_LARGE 4
#define NSA_FILL_FOLDED 5

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (a zero count, 3 * n_faces >= 2^31, n_boundary > 3 * n_faces) */
uint64_t nsa_mesh_fill_workspace(uint32_t n_faces, uint32_t n_boundary);

int nsa_mesh_fill_loops(const float *verts, const float *colors, uint32_t n_verts, const int32_t *faces, const int32_t *names,
                        uint32_t n_faces, const int32_t *edge_count, const int32_t *edge_forward, const int32_t *edge_start,
                        const int32_t *edge_halfedges, const int32_t *face_edges, const uint64_t *edge_totals, uint32_t n_boundary,
                        int has_max_edges, uint64_t max_edges, int has_max_size, double max_size2, uint32_t rings, uint32_t max_rings,
                        int skip_folded, void *workspace, int32_t *halfedges, int32_t *next, uint8_t *flags, int32_t *leader,
                        int32_t *rank, int32_t *order, int64_t *loop_ints, double *loop_reals, uint64_t *totals, nsa_stream_t stream);

int nsa_mesh_fill_emit(const float *verts, const float *colors, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                       const int32_t *order, uint32_t n_boundary, const int64_t *loop_ints, const double *loop_reals,
                       const uint64_t *totals, uint64_t n_new_verts, uint64_t n_new_faces, float *new_verts, float *new_colors,
                       int32_t *new_faces, nsa_stream_t stream);

/* ---- Section 24: minimum-area patches for holes that are not star-shaped (csrc/mesh_fill_area.hip) ---- */

/* Triangulates boundary loops of Section 23 without a new vertex, minimum total area first, after nsa_mesh_fill_loops on the same
 * arrays.  A loop of n edges has the vertices p_0 .. p_{n-1}, the start vertices of its half-edges in rank order; its patch has n - 2
 * faces.  tests/fill_area_ref.py restates this section in numpy and the device equals it element for element, bit for bit.
 *
 * Arithmetic.  Float64 on the fp32 positions; + - * rounded one by one, nothing contracted; Section 23's dot and cross products; one
 * square root per triangle, which must be IEEE correctly rounded: the device's sqrt(double) is (tests/test_mesh_fill_area_gpu.py pins
 * it against numpy on 10^5 values, half of them beside a rounding boundary), so none is written out here.
 *
 * Weight.  a = p_j - p_i, b = p_k - p_i, c = a x b, n2 = c . c, e = the largest of a . a, b . b, (b - a) . (b - a) (a running
 * "if x > e: e = x" from a . a).  T(i, j, k) = 0.5 * sqrt(n2) when n2 > min_sin2 * (e * e), +inf otherwise; min_sin2 is squared by
 * the caller.  A collinear run of loop vertices therefore gets no zero-area face for free.
 *
 * Table, for 0 <= i < k < n.  W[i][i+1] = 0; W[i][k] = the minimum over i < j < k of (W[i][j] + W[j][k]) + T(i, j, k); J[i][k] is the
 * smallest j that attains it (i + 1 when every candidate is +inf).  The minimum is over (value, j) pairs, a pair winning on a smaller
 * value or an equal value and a smaller j: associative and commutative, so every order of reduction gives the same bits.
 *
 * Forbidden chords.  A pair (i, k) that is no loop edge (k = i + 1, or (0, n - 1)) is a chord.  It is FORBIDDEN when Section 18's
 * edges (sorted by (lo, hi); found by bisection) hold the edge between the names of p_i and p_k, names being the face list the edge
 * table was built from, or when the two names are equal or invalid; its W[i][k] is +inf, set after the minimum is taken (J stays).
 * A patch then never puts a third face on an edge of the mesh.
 *
 * Class of a loop (area_ints column 0): -1 not selected (its Section 23 class c has bit c of class_mask clear); AREA_FILLED 0;
 * AREA_TOO_MANY_EDGES 1 (n > max_area_edges: nothing is computed); NO_TRIANGULATION 2 (n < 3, known to the plan, or W[0][n-1] not
 * finite, known after the tables).  The loop stays open in the last two.
 *
 * nsa_mesh_fill_area_plan (one launch): area_ints[B, 6] int64, the first L rows {class, n, table_offset, plan_face_offset,
 * row_offset, 0}: the exclusive scans of n^2, n - 2 and n over the loops that take a table (selected, 3 <= n <= max_area_edges), and
 * plan_totals[8] (uint64, device) {selected, loops with a table, too many edges, cells = sum n^2, max n, plan faces = sum (n - 2),
 * rows = sum n, 0}.  The caller reads plan_totals back once, sizes the workspace with nsa_mesh_fill_area_workspace(cells, rows) and
 * new_faces[plan faces, 3], and passes the numbers on.
 *
 * nsa_mesh_fill_area_tables: positions and names per row; chord mask and start values per cell; one launch per diagonal
 * d = 2 .. max n - 1 over the cells (i, i + d) of all tabled loops; then the final classes, area[B] (W[0][n-1]; 0 without a table),
 * area_ints column 5 = face_offset, the exclusive scan of n - 2 over the AREA_FILLED loops, and final_totals[4] {area_filled,
 * area_too_many_edges, no_triangulation, faces}; then the faces.  Face numbering is pre-order: the sub-tree of (i, k) holds k - i - 1
 * triangles; with j = J[i][k] the triangle (i, j, k) has number base, the sub-tree of (i, j) starts at base + 1 and that of (j, k)
 * at base + 1 + (j - i - 1); the root (0, n - 1) has base = the loop's offset.  The triangle is written (p_k, p_j, p_i), against the
 * boundary half-edges, naming the vertices the half-edges name.  new_faces is written in the PLAN's numbering (plan_face_offset):
 * the n - 2 rows of a loop that turned out NO_TRIANGULATION are (-1, -1, -1), and the caller drops them, which gives the final
 * numbering (face_offset).  Emit is one lane per face descending from the root, so no stack and no order of emission exists.
 *
 * Workspace: W and its transposed copy (float64 per cell), J (int32 per cell), the mask (a byte per cell), and per row the position
 * (3 float64), the loop and the name; in the order W, transposed W, positions, J, row loops, row names, mask, each part rounded up
 * to 256 bytes (the tests read W, J and the mask there).  NULL arguments (names excepted), max_area_edges = 0 or > 16384, class_mask >= 64, a negative
 * or NaN min_sin2, counts outside Section 23's ranges, cells / rows / max_n that cannot belong together (max_n < 3 or > 16384,
 * rows > n_boundary, cells < max_n^2 or > 16384 rows, faces > rows): NSA_EBADARG before anything is launched.  All four counts zero
 * (no tabled loop) launches nothing and returns 0.  Nothing is allocated or synchronised; no atomics. */

#define NSA_FILL_AREA_FILLED 0
#define NSA_FILL_AREA_TOO_MANY_EDGES 1
#define NSA_FILL_AREA_NO_TRIANGULATION 2

int nsa_mesh_fill_area_plan(const int64_t *loop_ints, const uint64_t *fill_totals, uint32_t n_faces, uint32_t n_boundary,
                            uint32_t class_mask, uint32_t max_area_edges, int64_t *area_ints, uint64_t *plan_totals, nsa_stream_t stream);

/* bytes of workspace (256-byte aligned, device); 0 for counts that cannot belong together */
uint64_t nsa_mesh_fill_area_workspace(uint64_t n_cells, uint64_t n_rows);

int nsa_mesh_fill_area_tables(const float *verts, uint32_t n_verts, const int32_t *faces, const int32_t *names, uint32_t n_faces,
                              const int32_t *edges, const uint64_t *edge_totals, const int32_t *order, uint32_t n_boundary,
                              const int64_t *loop_ints, const uint64_t *fill_totals, int64_t *area_ints, uint64_t n_cells, uint64_t n_rows,
                              uint32_t max_n, uint64_t n_new_faces, double min_sin2, void *workspace, double *area, int32_t *new_faces,
                              uint64_t *final_totals, nsa_stream_t stream);

/* out[i] = the square root of x[i] exactly as the weights take it (float64, device arrays of n): the hook of the test that holds the
 * device's root to IEEE rounding.  n = 0 launches nothing. */
int nsa_mesh_fill_area_roots(const double *x, uint64_t n, double *out, nsa_stream_t stream);

/* ---- Section 25: self-intersections of a mesh, decided exactly (csrc/mesh_intersect.hip) ---- */

/* Which pairs of faces of a mesh meet.  The vertices are fp32, every fp32 number is a rational, so for two faces A and B (closed
 * triangles) the set I = A n B is defined over the reals and so is everything below: the answer is that real-number answer, for
 * every pair, without a tolerance.  tests/intersect_ref.py constructs I in rationals and the device equals it element for element.
 *
 * Usable faces: Section 14's (cause 0), minus the faces whose three vertices are exactly collinear -- the float64 cross product of
 * Section 14 is not exact, so 256-bit integers decide -- state 4, skipped and counted like causes 1 .. 3.  State 5: the exponents of
 * the face's own nine coordinates span more than 102 binades; the device leaves the face out and the caller decides it.
 *
 * Candidates: the pairs i < j of usable faces whose exact boxes (the fp32 min / max of the nine coordinates, no pad) overlap as closed
 * boxes on all three axes; with `side` (a byte per face) only those with side[i] != side[j].  Their number, and its split by s, are
 * functions of the inputs.
 *
 * s = the number of vertex POSITIONS of A that are vertex positions of B (fp32 equality, -0 = +0), 0 .. 3: a seam with repeated
 * vertices behaves like a welded one.  A candidate is REPORTED iff I contains a point outside the convex hull of the shared positions:
 * s = 0: I is not empty; s = 1: I is more than the shared vertex; s = 2: I is more than the shared edge (the coplanar fold-over);
 * s = 3: always (a duplicate, in either orientation).  Ordinary neighbours of a manifold mesh are never reported.
 *
 * code of a reported pair: bits 0-1 the kind -- NSA_ISECT_PROPER: the relative interiors of A and B meet (a transversal crossing, a
 * coplanar overlap with area, a fold-over, a duplicate); NSA_ISECT_TOUCH: reported and not proper (a vertex on a face, an edge lying
 * in a face, a T-junction along part of an edge, two edges crossing at a point); NSA_ISECT_UNRESOLVED: the exponents of the pair's 18
 * coordinates span more than 59 binades, the 256-bit determinants could overflow, and the caller decides the pair --; bit 2
 * NSA_ISECT_COPLANAR; bits 4-5 s.
 *
 * Stages.  1: orientation determinants of four points in float64 (+ - * one by one, nothing contracted) with the forward error bound
 * 2^-49 * permanent derived in csrc/intersect_passes.hpp; a sign is certain when |det| > bound or bound == 0.  Stage 1 decides a pair
 * only from signs that are certain and not zero: a pair with s = 0 and all signs generic, and any pair in which every vertex of one
 * face that is no shared position lies strictly on one side of the other's plane (not reported).  2: the same determinants in 256-bit
 * two's-complement integers on the coordinates scaled by a power of two, zeros included, and the closed-set decision of
 * intersect_passes.hpp for every s, the coplanar case included.
 *
 * nsa_tri_isect_count, on the tree nsa_tri_ray_build made for the same arrays: state[F]; then one lane per sorted face walks the tree
 * (its padded boxes are supersets of the exact ones; the exact-box clause is part of the pair test, so the walk and the brute force
 * of NSA_ISECT_BRUTE agree by construction) and counts its records; then totals[16] (uint64, device): {records to emit, candidates
 * with s = 0, 1, 2, 3, candidates decided by stage 1, by stage 2, left unresolved, faces of state 1, 2, 3, 4, 5, usable faces, 0, 0}.
 * The caller reads totals back, sizes pairs[n, 2] (int64) and code[n] and calls nsa_tri_isect_emit with the same arguments, which
 * writes the records (i, j), i < j, grouped by lane in walk order: sorting by i * F + j gives the canonical order.  No atomics; two
 * runs write the same bytes.
 *
 * Workspace: count (uint32 per face), offset (uint64, F + 1), statistics (8 uint32 per face), each part rounded up to 256 bytes.
 * A count above 2^31 - 1, an unknown flag, a NULL array (side excepted) with n_faces > 0: NSA_EBADARG before anything is launched.
 * n_faces = 0 (and, for emit, n_pairs = 0) launches nothing and returns 0.  Nothing is allocated or synchronised. */

#define NSA_ISECT_PROPER 1
#define NSA_ISECT_TOUCH 2
#define NSA_ISECT_UNRESOLVED 3
#define NSA_ISECT_COPLANAR 4
#define NSA_ISECT_BRUTE 1u /* flags: test all pairs of usable faces instead of walking the tree */

/* bytes of workspace (256-byte aligned, device); 0 for n_faces = 0 or above 2^31 - 1 */
uint64_t nsa_tri_isect_workspace(uint32_t n_faces);

int nsa_tri_isect_count(const void *tree, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                        const uint8_t *side, uint32_t flags, void *workspace, uint8_t *state, uint64_t *totals, nsa_stream_t stream);

int nsa_tri_isect_emit(const void *tree, const float *verts, uint32_t n_verts, const int32_t *faces, uint32_t n_faces,
                       const uint8_t *side, uint32_t flags, const void *workspace, const uint8_t *state, uint64_t n_pairs,
                       int64_t *pairs, uint8_t *code, nsa_stream_t stream);

/* ---- Section 26: one vertex per fan of faces -- cutting a mesh into a 2-manifold (csrc/mesh_manifold.hip) ---- */

/* The "cutting" step of Gueziec et al.: every vertex is duplicated once per FAN of faces around it, the fans found through regular
 * edges only.  After nsa_mesh_edges (Section 18) on the same faces (and the same mask), from the arrays it wrote and its totals as
 * they lie on the device.  Everything is by index: coordinates play no part.  Integer work, exact and bit-reproducible.
 * tests/manifold_ref.py restates this statement sequentially.  n_verts + 3 * n_faces < 2^31 (V below is n_verts, F n_faces).
 *
 * Corners.  Corner c = 3 f + k of a contributing face f (Section 18's rule: face_edges[3 f] >= 0) sits at vertex faces[f][k].
 *
 * Regular edge.  edge_count == 2; with NSA_SPLIT_CUT_INCONSISTENT in flags, edge_forward == 1 as well; with face_label (int32 [F],
 * NULL = none) given, both faces carry the same label (so a caller can cut seams between labelled patches).  Every other edge with
 * edge_count >= 2 is CUT.
 *
 * Fans.  Two corners at the same vertex are joined when their faces share a regular edge incident to that vertex; the fans are
 * the classes of the transitive closure.  The LEADER of a fan is its smallest corner id.  One union-find over the 3 F corners with
 * Section 11's uf_find / uf_unite unchanged, one pass over the edges: a regular edge (lo, hi) unites its two faces' corners at lo,
 * and their corners at hi.  parent[x] <= x, so the root is the leader whatever the interleaving and the atomics decide nothing.
 *
 * Naming.  The leaders in ascending corner order, stably argsorted by vertex: ascending (vertex, leader).  The first fan of vertex v
 * keeps the name v; every further fan gets V + r, r its rank among all further fans in that order (one exclusive scan of the "not
 * head of its run" flags).
 *
 * Outputs.
 *   corner_fan[3 F] int32    the leader of the corner's fan, -1 for a corner of a face that does not contribute
 *   vertex_fans[V] int32     the number of fans of each vertex, 0 for an unused one
 *   faces_out[F, 3] int32    contributing faces renamed by fan; another face is copied, except that an index >= V is written as -1,
 *                            so that no such face reaches a new vertex by accident
 *   new_source[3 F] int32    the first n_new entries are valid: entry r is the vertex that new vertex V + r copies
 *   totals[8] (uint64, device; the caller reads them once):
 *     {contributing faces, fans, singular vertices (more than one fan), of those the ones with no cut edge incident (a pinch only),
 *      cut edges, n_new, the most fans at one vertex, status}
 * status: Section 11's bits from the union-find; 0 unless the implementation is wrong.
 *
 * Properties (proved in DESIGN 4y).  The link of a vertex v is the graph whose nodes are the edges at v and whose arcs are the
 * corners at v, each joining its face's two edges at v.  A node of degree above two is an edge with more than two faces, which is
 * cut; so cutting the link at every node whose edge is not regular leaves nodes of degree <= 2 only: paths and cycles.  Hence (a) a
 * fan holds at most two faces on any input edge, (b) every edge of the output has edge_count <= 2, (c) every output vertex has
 * exactly one fan, and the operation is idempotent: on its own output it finds no cut edge, n_new = 0 and faces_out = faces.  Old
 * vertices and every face index keep their place (a face's k-th index stays its k-th).  The result is a function of (faces, n_verts,
 * face_mask, flags, face_label) alone.
 *
 * Kernel shape: the join over the edges; the leader pass over the corners, which also gives every corner its key -- its vertex when
 * it leads, n_verts otherwise, which sorts last; one stable radix argsort (Section 4's) of the 3 F keys with only the 8-bit passes
 * n_verts needs; run heads by comparing neighbours in the sorted order; one exclusive scan; the face rewrite.  Totals are sums, ORs and
 * one maximum of per-block integers; there are no atomics outside the union-find.  No attribute is touched: the caller gathers rows
 * by new_source.
 *
 * NULL faces, table array, workspace, totals or output array (vertex_fans may be NULL when n_verts = 0), an unknown flag, or
 * n_verts + 3 * n_faces >= 2^31: NSA_EBADARG before anything is launched.  n_faces = 0 launches nothing, writes nothing and returns
 * 0.  Arrays that nsa_mesh_edges did not write for these faces give meaningless fans, never an access out of bounds.  Nothing is
 * allocated or synchronised. */

#define NSA_SPLIT_CUT_INCONSISTENT 1u /* flags: an edge whose two faces traverse it the same way is cut as well */

/* bytes of workspace (256-byte aligned, device); 0 for an invalid count (n_faces = 0 or n_verts + 3 * n_faces >= 2^31) */
uint64_t nsa_mesh_split_fans_workspace(uint32_t n_verts, uint32_t n_faces);

int nsa_mesh_split_fans(const int32_t *faces, uint32_t n_faces, uint32_t n_verts, const int32_t *face_label, uint32_t flags,
                        const int32_t *edges, const int32_t *edge_count, const int32_t *edge_forward, const int32_t *edge_start,
                        const int32_t *edge_halfedges, const int32_t *face_edges, const uint64_t *edge_totals, void *workspace,
                        int32_t *corner_fan, int32_t *vertex_fans, int32_t *faces_out, int32_t *new_source, uint64_t *totals,
                        nsa_stream_t stream);

/* ---- Section 27: point-to-plane registration -- the moved source and the 6x6 normal equations (csrc/mesh_register.hip) ---- */

/* One iteration of point-to-plane ICP (Chen & Medioni 1992; open3d's TransformationEstimationPointToPlane with a RobustKernel) is:
 * move the float64 source, query its correspondences with Section 8's or Section 15's query, and sum the rows of the linearised
 * problem.  This section is the first and the last of the three; the 6x6 solve is the caller's (nicer_slam_amd/mesh_register.py states
 * it).  Everything is float64 with every operation rounded on its own (no fused multiply-add), and the order of every sum is a function
 * of n alone: the results are the same bits on every run and every device, and tests/register_ref.py restates them in numpy.
 *
 * nsa_icp_transform.  cur [n, 3] float64 is moved in place by the row-major 4x4 upd (16 doubles in HOST memory, read before the call
 * returns): y_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k.  cur32 [n, 3] receives the fp32 rounding of the result, which the queries take.
 *
 * nsa_icp_plane_system.  One row per source point i, p = cur[i].  corr [n] int32 names the row's correspondence:
 *   NSA_ICP_CLOUD    corr = idx of nsa_nn_query.  With 0 <= corr < n_targets: q = targets[corr] and nrm = normals[corr] (fp32 [n_targets, 3],
 *                    widened), and dd = d * d with d = dist[i] (the query's fp32 distance, widened).
 *   NSA_ICP_SURFACE  corr = face of nsa_tri_query_bounded.  With 0 <= corr < n_faces and the face's three indices in [0, n_verts):
 *                    q = closest[i] (the query's fp32 closest point, widened), dd = d2[i] (the query's float64 squared distance), and
 *                    nrm = c / sqrt((c_x c_x + c_y c_y) + c_z c_z) with c = ab x ac in float64 from the face's fp32 vertices
 *                    (c_x = ab_y ac_z - ab_z ac_y and so on; the root and the quotients correctly rounded).
 * Any other corr: the row has no correspondence.  A row with one is USED when nrm is finite and not (0, 0, 0).  Per used row:
 *   d = p - q;  r = (n_x d_x + n_y d_y) + n_z d_z;  a = (p_y n_z - p_z n_y, p_z n_x - p_x n_z, p_x n_y - p_y n_x);  J = (a, nrm)
 *   w = 1 (NSA_ICP_KERNEL_L2);  1 if |r| <= k else k / |r| (HUBER);  v v with u = r / k, v = 1 - u u if |r| <= k else 0 (TUKEY)
 *   g_i = w J_i
 * sums [30] (float64, device):  [0..20] g_i J_j for i <= j, the upper triangle row by row;  [21..26] g_i r;  [27] r r;  [28] (w r) r;
 * [29] dd, over the rows with a correspondence, used or not.  counts [2] (uint64, device): rows with a correspondence, rows used.
 * r and J change sign together with nrm, so none of the sums depends on the side the normals point to.
 *
 * Order.  Tiles of 4096 consecutive rows.  Lane l of 256 adds the rows l, l + 256, ... of its tile in ascending order onto +0.0; a row
 * that is past n, has no correspondence or is not used adds +0.0 in its place, so the order does not depend on which rows matched.  A
 * binary tree over the 256 lanes, s[i] = s[2 i] + s[2 i + 1], eight levels, gives the tile's total.  While more than one value is left,
 * the values go in groups of 256 consecutive ones, the last group padded with +0.0, through the same tree.  No floating-point atomic
 * takes part and nothing depends on the launch geometry or on the order in which workgroups finish.
 *
 * n >= 2^31, an unknown mode or kernel, k not positive and finite for HUBER or TUKEY, or (for n > 0) a NULL array of the mode, NULL
 * workspace, sums or counts: NSA_EBADARG before the device is touched.  n = 0 launches nothing, writes nothing and returns 0.  Nothing
 * is allocated or synchronised; the workspace is a function of n.  An index outside its range makes a row without a correspondence,
 * never an access out of bounds. */

#define NSA_ICP_CLOUD 0
#define NSA_ICP_SURFACE 1
#define NSA_ICP_KERNEL_L2 0
#define NSA_ICP_KERNEL_HUBER 1
#define NSA_ICP_KERNEL_TUKEY 2

int nsa_icp_transform(double *cur, uint32_t n, const double *upd, float *cur32, nsa_stream_t stream);

/* bytes of workspace (256-byte aligned, device); 0 for n = 0 or n >= 2^31 */
uint64_t nsa_icp_plane_system_workspace(uint32_t n);

int nsa_icp_plane_system(const double *cur, uint32_t n, int mode, const int32_t *corr, const float *dist, const float *targets,
                         const float *normals, uint32_t n_targets, const double *d2, const float *closest, const float *verts,
                         uint32_t n_verts, const int32_t *faces, uint32_t n_faces, int kernel, double k, void *workspace, double *sums,
                         uint64_t *counts, nsa_stream_t stream);

/* ---- Section 28: k nearest neighbours and normals of raw clouds (csrc/mesh_eval.hip, csrc/cloud_normals.hip) ---- */

/* nsa_nn_query_k.  index: one built by nsa_nn_build over n_targets targets (Section 8).  With the fp32 d2 of Section 8,
 * (dx * dx + dy * dy) + dz * dz with every operation rounded on its own, row j of idx / dist [n_queries, k] receives the k smallest
 * targets of query j under the total order (d2, target index), in that order: an exact tie goes to the lower index, at the k-th
 * place too, and neither the set nor the order depends on the order the index's cells are read in.  dist is the correctly rounded
 * fp32 root of d2.  With a finite max_dist only targets with d2 < (float)(max_dist * max_dist) count (strict, as nsa_nn_query).
 * count [n_queries] receives the number found, min(k, accepted targets); the slots behind it hold (-1, +inf).  Targets with a
 * non-finite coordinate are never returned.  A non-finite query gives count 0 and (-1, NaN) in every slot.  k = 1 writes what
 * nsa_nn_query writes.
 *
 * 1 <= k <= 64 and max_dist > 0, else NSA_EBADARG; n_queries > 0 with a NULL queries, idx, dist or count: NSA_EBADARG before anything
 * is launched; n_queries = 0 launches nothing and returns 0.  Nothing is allocated or synchronised. */
int nsa_nn_query_k(const void *index, uint32_t n_targets, const float *queries, uint32_t n_queries, uint32_t k, double max_dist,
                   int32_t *idx, float *dist, uint32_t *count, nsa_stream_t stream);

/* nsa_cloud_normals.  One row per neighbourhood i < m: the first c = count[i] slots of idx[i] ([m, k] int32) name points of the cloud
 * points [n, 3], in the order nsa_nn_query_k wrote them.  All in float64 from the fp32 coordinates, every operation rounded on its own:
 *   mu_a = ((((+0 + p_0a) + p_1a) + p_2a) + ...) / c;  d_j = p_j - mu;  S_ab = ((+0 + d_0a d_0b) + d_1a d_1b) + ...   (two passes)
 *   cyclic Jacobi on S with V = I: pivots (p, q) = (0, 1), (0, 2), (1, 2) per sweep, g = a_pq.  g == 0: skipped.
 *   |a_pp| + |g| == |a_pp| and |a_qq| + |g| == |a_qq|: a_pq = 0 without a rotation.  Else theta = (a_qq - a_pp) / (2 g),
 *   t = 1 / (|theta| + sqrt(theta theta + 1)) (1 / (|theta| + |theta|) when |theta| > 2^500), negated when theta < 0,
 *   c = 1 / sqrt(t t + 1), s = t c, h = t g;  a_pp -= h, a_qq += h, a_pq = 0;  with r the third index (a_rp, a_rq) = (c a_rp - s a_rq,
 *   s a_rp + c a_rq);  for each row i of V (v_ip, v_iq) = (c v_ip - s v_iq, s v_ip + c v_iq).  The sweeps end with the first one that
 *   finds the three off-diagonals zero, or after 16.
 *   eigenvalues [m, 3] (may be NULL): the diagonal, ascending; equal values keep the order of their columns; a NaN is the quiet NaN
 *   0x7FF8000000000000.  The normal is the column v of the smallest, v / sqrt((v_x v_x + v_y v_y) + v_z v_z), negated when
 *   viewpoint_rows = 0 and its component of largest magnitude (ties: the lowest axis) is negative, or when viewpoint_rows > 0 and
 *   ((n_x e_x + n_y e_y) + n_z e_z) < 0 with e = w - origin[i] and w = viewpoint[0] (viewpoint_rows = 1) or viewpoint[i]
 *   (viewpoint_rows = m); then rounded once to fp32.
 * valid [m] = 1 when 3 <= c <= k, every one of the c indices lies in [0, n), the three eigenvalues are finite and the middle one is
 * > 0; otherwise 0 and the normal is (0, 0, 0), which nsa_icp_plane_system does not use.  A row with c = 0, c > k or an index outside
 * [0, n) reads no point and has NaN eigenvalues.  tests/normals_ref.py restates all of it in numpy.
 *
 * k outside [1, 64], n or m >= 2^31, viewpoint_rows not 0, 1 or m: NSA_EBADARG.  m = 0 launches nothing and returns 0.  For m > 0 a NULL
 * idx, count, origin, normals or valid, a NULL points with n > 0 or a NULL viewpoint with viewpoint_rows > 0: NSA_EBADARG before
 * anything is launched. */
int nsa_cloud_normals(const float *points, uint32_t n, const int32_t *idx, const uint32_t *count, uint32_t m, uint32_t k,
                      const float *origin, const float *viewpoint, uint32_t viewpoint_rows, float *normals, double *eigenvalues,
                      uint8_t *valid, nsa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NICER_SLAM_AMD_H */
