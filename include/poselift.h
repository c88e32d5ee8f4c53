/* poselift.h -- C ABI of the MI355X (gfx950) 2D->3D pose-lifting train path.
 *
 * The reference (RHnejad/3D_PoseEstimation) has no FFI: its hot path is a plain
 * PyTorch nn.Module plus a script-level train step.  This header is therefore the
 * boundary a maintainer binds with ctypes; every entry point
 * names the reference lines whose computation it replaces.  All paths are relative
 * to the reference root.
 *
 * Conventions
 *   - plain C, POD arguments, no torch types; device pointers are hipMalloc'ed
 *     (or torch-owned) fp32 unless stated; every tensor is dense row-major.
 *   - the caller owns every buffer including the workspace; the library never
 *     allocates or frees device memory and keeps no device-side global state.
 *   - every call enqueues work on `stream` and returns; nothing synchronises.
 *   - return value: PL_OK (0) or a negative PLStatus; pl_last_error() gives the
 *     thread-local message.  Nothing throws across the ABI.
 *   - alignment: a device pointer that a kernel behind an entry point reads or
 *     writes 16 bytes at a time must be 16-byte aligned, else the call returns
 *     PL_EINVAL before any launch with a message naming the argument ("x not
 *     16-byte aligned").  A contiguous VIEW of a larger tensor (table + n * 34)
 *     need not be: copy it first.  Pointers only element code touches may sit at
 *     any 4-byte boundary.  DESIGN.md 3h lists every entry point and pointer.
 */
#ifndef POSELIFT_H_
#define POSELIFT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PL_VERSION 123 /* 0.1.23: + pl_camera_project, pl_camera_project_bwd, pl_camera_reproj_errors, pl_camera_reproj_loss_scratch_bytes, pl_camera_reproj_loss_fwd_bwd, pl_camera_fit_translation and their _host forms (cameras: projection with distortion, reprojection loss, root translation fitted to a 2-D track); 0.1.22: + pl_pose_errors_w, pl_pose_errors_w_host, pl_pose_metrics_w_scratch_bytes, pl_pose_metrics_accum_w (evaluation with missing joints: visibility-weighted alignment, masked sums and counts, per-joint visible counts); 0.1.21: + PLSkeleton, PLSkeletonCriterion, PL_CRIT_HAS_SKELETON, pl_bone_lengths, pl_skeleton_terms_host, pl_skeleton_abi_bytes (bone-length and left/right symmetry terms of the criterion, one launch more per step); 0.1.20: + PLEma, PLAdamWStep.ema, pl_adamw_flat_planes_clip_ema, pl_swap_f32 (averaged weights kept inside the AdamW launches); 0.1.19: + pl_lifter_bwd_slab_rides (how many split-K sums of weight gradients ride in chained GEMM launches); 0.1.18: + PLPoseCrop, pl_pose_augment_gather_crop, pl_pose_augment_gather_crop_t, pl_pose_augment_host_crop, pl_pose_augment_host_crop_t, pl_frame_warp_gather_crop, pl_frame_warp_host_crop, pl_pose_crop_boxes, pl_pose_crop_boxes_host, pl_crop_poses, pl_crop_poses_host (person-centred crop from each row's 2-D pose inside the two batch launches); 0.1.17: + PLCriterion, pl_pose_loss_scratch_bytes, pl_pose_loss_fwd_bwd, pl_lifter_train_fwd_bwd_crit, pl_lifter_train_step_crit (the train step's criterion: mse, l1, smooth_l1, mpjpe, weighted per joint); 0.1.16: + pl_pose_prepare, pl_pose_stats, pl_pose_affine and their _host forms, pl_pose_stats_scratch_bytes, pl_pose_stats_chunk_rows, pl_pose_augment_gather_t, pl_pose_augment_host_t, pl_pose_errors_t, pl_mpjpe_accum_t (pose tables: prepare, statistics, the per-column transform and its way back inside the batch, error and metric launches); 0.1.15: + PLFrameWarp, pl_frame_warp_gather, pl_frame_warp_host (frame gather + resize + the pose augmentation's warp in one launch); 0.1.14: + PLPoseAug, pl_pose_augment_gather, pl_pose_augment_host (seeded train-time pose augmentation inside the batch gather); 0.1.13: + PLClipRecord, pl_grad_norm_scratch_bytes, pl_grad_norm_clip, pl_adamw_flat_clip, pl_adamw_flat_dev_clip, pl_adamw_flat_planes_clip (gradient-norm clipping and non-finite skip on the device); 0.1.12: + pl_pose_errors, pl_pose_errors_host, pl_pose_metrics_scratch_bytes, pl_pose_metrics_accum (evaluation: MPJPE / N-MPJPE / P-MPJPE, PCK counts, per group); 0.1.11: + pl_vit_*_bf16, pl_vit_bf16_pack (MyViT "bf16p": bf16 operand carriers written by their producers); 0.1.10: + pl_vit_* (the MyViT transformer lifter); 0.1.9: + pl_conv2d_planes_fwd_hw, pl_conv2d_planes_wgrad_hw (the stem on the planes GEMM); 0.1.8: + pl_lifter_train_step, pl_lifter_step_carries_adamw; 0.1.7: + pl_workspace_bitmap_format (small-batch layer kernels); 0.1.6: + pl_counter_add; 0.1.5: + pl_flip_pose_ex, pl_flip_w_nhwc (phase5 Flip branch); 0.1.4: + pl_planes_split_strided; 0.1.3: + pl_bn_join_bwd (0.1.2: operand-plane outputs of the BatchNorm / join kernels, pl_gemm_planes_raw) */

typedef enum PLStatus {
  PL_OK = 0,
  PL_EINVAL = -1,       /* null pointer / bad enum / misaligned pointer          */
  PL_ESHAPE = -2,       /* unsupported shape (hidden % 4 != 0, dims <= 0, ...)   */
  PL_EDTYPE = -3,       /* unsupported compute dtype                             */
  PL_EBATCH = -4,       /* B < 2 with training-mode BatchNorm (torch raises too) */
  PL_EHIP = -5,         /* a HIP runtime call or launch failed                   */
  PL_EWORKSPACE = -6,   /* workspace pointer null or too small                   */
  PL_ESYNC = -7         /* the PLSync gather callback reported a failure         */
} PLStatus;

/* arithmetic (and operand storage) of the 1024-wide GEMMs:
 *   PL_F32     v_mfma_f32_32x32x2_f32, exact fp32 products                  (meets the 1e-3 mm gate)
 *   PL_BF16    operands rounded to bf16, v_mfma_f32_32x32x16_bf16           (~1 mm MPJPE).  On whole 128-tiles with
 *              BatchNorm the operands are STORED as bf16 by their producers (activations, dz, a bf16 weight shadow)
 *              and staged by LDS-DMA; z, the gradient flow and every reduction stay fp32.  Other shapes keep fp32
 *              storage and round while staging: the same values, the same products.
 *   PL_BF16X6  each fp32 operand split into 3 bf16 pieces, 6 bf16 MFMAs per product term:
 *              fp32-grade results (meets the gate too) at 6/16 of the fp32 matrix time
 *   PL_F16X3   fp32-grade on HALF the matrix work of PL_BF16X6: every operand tensor is written by its producing
 *              kernel as two fp16 planes, S x = h + l / 2048 (h = fp16(S x), l = fp16((S x - h) 2048), S a per-tensor
 *              power of two: 22-23 significant bits), and a b = h_a h_b + (h_a l_b + l_a h_b) / 2048 is accumulated on
 *              two fp32 accumulators by three fp16 MFMAs; the GEMM stages the planes with LDS-DMA and does no split
 *              work.  Whole 128-tiles with BatchNorm and local statistics; other shapes run PL_BF16X6 arithmetic. */
typedef enum PLDtype { PL_F32 = 0, PL_BF16 = 1, PL_BF16X6 = 2, PL_F16X3 = 3 } PLDtype;

/* Cross-rank BatchNorm statistics ("SyncBN"; data-parallel extension, SURVEY 8e -- the reference is
 * single-process and has no counterpart).  With PLDesc.sync set and world > 1, training-mode BatchNorm
 * normalises with the statistics of the GLOBAL batch (world x B rows; every rank must pass the same B):
 * after a layer's partial statistics are computed the library calls
 *     gather(user, buf, floats_per_rank, stream)
 * where buf = [world][floats_per_rank] device floats inside the caller's workspace and slab `rank` is
 * already filled by work enqueued on `stream`.  The callee must enqueue an all-gather that fills the
 * other slabs, ordered after that work and before anything enqueued on `stream` later (RCCL:
 * ncclAllGather in place on that stream), and return 0 (non-zero -> PL_ESYNC).  One gather per hidden
 * layer in the training forward (2 x ceil(B/64)-ish x hidden floats) and one in backward.  The merged
 * result does not depend on how the global batch is cut into ranks: forward activations and running
 * statistics are bit-identical to one process running the concatenated batch. */
typedef int (*PLGatherFn)(void* user, float* buf, int64_t floats_per_rank, void* stream);
typedef struct PLSync {
  int32_t world;       /* number of ranks (1 = local statistics)              */
  int32_t rank;        /* this process, 0 <= rank < world                     */
  PLGatherFn gather;
  void* user;          /* passed back to gather                               */
} PLSync;

/* Lifter descriptor: LinearModel(i_dim, o_dim, linear_size, num_stage, p_dropout, BN)
 * phase1_lifting/baselineModel.py:50-85.
 *
 * params     flat fp32 parameter arena.  Tensors appear in the reference's
 *            parameters() order -- per hidden layer: Linear.weight [out][in],
 *            Linear.bias, BatchNorm.weight, BatchNorm.bias (BN tensors are present
 *            even when bn == 0, as in the reference) -- then w2.weight, w2.bias.
 *            Every tensor starts at a multiple of 64 floats: pl_param_offset().
 * bn_running [n_hidden][2][hidden] fp32: running_mean then running_var per layer.
 * bn_batches [n_hidden] int64 num_batches_tracked, or NULL.
 */
typedef struct PLDesc {
  int32_t in_dim;      /* 34 = 17 joints x 2                                  */
  int32_t hidden;      /* linear_size, multiple of 4                          */
  int32_t out_dim;     /* 51 = 17 joints x 3                                  */
  int32_t num_stage;   /* residual blocks; hidden layers = 1 + 2*num_stage    */
  int32_t bn;          /* BN flag of the reference constructor                */
  int32_t dtype;       /* PLDtype: arithmetic of the 1024-wide GEMMs          */
  float p_dropout;     /* nn.Dropout p                                        */
  float bn_eps;        /* 1e-5 (nn.BatchNorm1d default)                       */
  float bn_momentum;   /* 0.1                                                 */
  int32_t reserved;
  float* params;
  float* bn_running;
  int64_t* bn_batches;
  const PLSync* sync;  /* NULL = BatchNorm over the local batch (the reference's behaviour) */
  /* Graph replay (hipGraph / torch.cuda.graph capture of the train step; no reference counterpart): a device counter of
   * completed steps.  When set, pl_lifter_fwd_train's dropout stream uses step + *step_dev (the kernels read it), and
   * pl_lifter_train_fwd_bwd increments it once per call, after the forward's last reader -- so a captured step draws fresh
   * dropout masks on every replay.  NULL: the `step` argument alone (the eager behaviour). */
  const uint64_t* step_dev;
  /* Operand planes of the 1024-wide weights kept ACROSS calls (optional; caller-owned, pl_wplanes_bytes() bytes).
   * NULL: every forward call splits the weights into its workspace first.  Set: the planes live here; with
   * wplanes_valid != 0 the caller asserts they hold the current parameters (pl_adamw_flat_planes wrote them and nothing
   * changed the parameters since) and the forward reads them as they are; with 0 the forward refreshes them first. */
  void* wplanes;
  int32_t wplanes_valid;
  int32_t reserved2;
} PLDesc;

int pl_version(void);
const char* pl_last_error(void);

/* ---- arena layout (host only, no device work) ---------------------------------- */
int64_t pl_num_hidden(const PLDesc* d);               /* 1 + 2*num_stage            */
int64_t pl_param_tensors(const PLDesc* d);            /* 4*n_hidden + 2             */
int64_t pl_param_offset(const PLDesc* d, int64_t i);  /* floats, multiple of 64     */
int64_t pl_param_numel(const PLDesc* d, int64_t i);
int64_t pl_param_arena_floats(const PLDesc* d);       /* padded arena length        */
/* Workspace for B rows: saved activations, masks, BN statistics, gradient scratch.
 *
 * UNINITIALISED MEMORY.  The workspace, every `scratch` argument of this header and every output buffer may hold
 * anything on entry, non-finite bit patterns included: the library reads no word of them that an earlier launch of
 * the same call sequence (a forward before its backward, a backward before the optimizer step that takes its slabs)
 * did not write, and it uses no memset.  A result never depends on what these buffers held.  And the library never
 * writes outside the bytes it asked for: pl_workspace_bytes / pl_*_scratch_bytes bytes from the pointer it was given,
 * an output's own extent.  The one exception is the f16x3 range-guard record (PL_RANGE_SITES words, below), an
 * accumulator "zeroed by the caller"; state that calls accumulate into -- PLClipRecord's skipped count, the metric
 * sums and counts, an `out` a loss adds to, AdamW's moments -- is the caller's to initialise and is not scratch.
 * tests/test_gpu_scratch_independence.py holds both halves, bit for bit, for every kernel of csrc/: each __global__
 * function is launched by one of its cases or listed there as exempt, with the reason. */
size_t pl_workspace_bytes(const PLDesc* d, int64_t B);
/* Debug/test view into the workspace.  which: 0 z (pre-BN GEMM output), 1 act (layer
 * output incl. residual), 2 keep&relu bitmap, 3 batch mean, 4 batch rstd.           */
int pl_workspace_view(const PLDesc* d, int64_t B, int which, int64_t layer,
                      size_t* offset_bytes, size_t* size_bytes);
/* Layout of the bitmap of hidden layer `layer` after a training forward of B rows (which = 2 above):
 *   0  row format: [B][4*ceil(H/256)] words; row r, 256-column strip q, word j: bit l <-> column 256 q + 4 l + j;
 *   1  tile format (batches of <= 64 rows whose hidden layers run as ONE launch each, csrc/small_layer.hip): H words;
 *      element (r, c) is bit (r & 15) * 4 + ((c >> 2) & 3) of word (c >> 4) * 16 + (r >> 4) * 4 + (c & 3).
 * Negative = error code.  (Debug / test only: the backward pass knows by itself.)
 * pl_lifter_fwd_eval_saved takes none of the small-batch launches: it writes format 0 at every B, whatever this returns. */
int pl_workspace_bitmap_format(const PLDesc* d, int64_t B, int64_t layer);

/* ---- forward ------------------------------------------------------------------- */
/* model.eval(); model(x)   phase1_lifting/baselineModel.py:87-102 under
 * train_1.py:112-126 (BatchNorm on running statistics, Dropout = identity).
 * x [B][in_dim], y [B][out_dim]. */
int pl_lifter_fwd_eval(const PLDesc* d, const float* x, float* y, int64_t B,
                       void* workspace, size_t workspace_bytes, void* stream);

/* model.train(); model(x)  phase1_lifting/baselineModel.py:87-102 under train_1.py:86.
 * Updates bn_running / bn_batches like nn.BatchNorm1d (momentum, unbiased running
 * var).  Dropout keep decisions come from the Philox4x32-10 stream keyed by
 * (seed, step, layer, element) documented in csrc/philox.h, or -- parity mode --
 * from inject_keep: n_hidden bitmaps laid out like workspace view 2 (NULL = Philox).
 * Saves what pl_lifter_bwd needs in the workspace. */
int pl_lifter_fwd_train(const PLDesc* d, const float* x, float* y, int64_t B,
                        void* workspace, size_t workspace_bytes,
                        uint64_t seed, uint64_t step, const uint64_t* inject_keep,
                        void* stream);

/* loss.backward() through the module (autograd of baselineModel.py:87-102).
 * dy [B][out_dim]; flat_grads: arena shaped like d->params, OVERWRITTEN with the
 * gradient of every parameter; dx [B][in_dim] or NULL (phase5_loop needs it,
 * train_1.py does not). Must follow pl_lifter_fwd_train on the same workspace. */
int pl_lifter_bwd(const PLDesc* d, const float* x, const float* dy, int64_t B,
                  void* workspace, size_t workspace_bytes, float* dx,
                  float* flat_grads, void* stream);

/* model.eval() with gradients flowing through it (phase5_loop/train_5.py:120 runs the lifter in eval mode inside the cycle
 * graph): the eval forward computed so that its backward can follow -- BatchNorm on the running statistics (left
 * untouched), Dropout = identity, pre-activations and ReLU bitmaps saved in the workspace -- and that backward: dx and
 * the gradient of every parameter (dgamma, dbeta included, as torch computes them in eval mode).  Same numbers as
 * pl_lifter_fwd_eval to fp32 round-off; pl_lifter_fwd_eval stays the fast path when nothing needs a gradient. */
int pl_lifter_fwd_eval_saved(const PLDesc* d, const float* x, float* y, int64_t B,
                             void* workspace, size_t workspace_bytes, void* stream);
int pl_lifter_bwd_eval(const PLDesc* d, const float* x, const float* dy, int64_t B,
                       void* workspace, size_t workspace_bytes, float* dx, float* flat_grads, void* stream);

/* The same backward restricted to a range of layers (data-parallel overlap, no reference
 * counterpart).  Layers are numbered along the chain: hidden Linears 0 .. L-1 (L = pl_num_hidden)
 * and the output Linear = L.  The call runs layers hi, hi-1, .., lo (0 <= lo <= hi <= L); the
 * gradient flowing between two calls lives in the workspace, so consecutive ranges
 * (L..a), (a-1..b), .., (c-1..0) == pl_lifter_bwd, bit for bit.  After the range ending at lo the
 * gradients of every tensor from pl_param_offset(d, 4*lo) to the end of the arena are final:
 * their all-reduce can run while the lower layers compute.  dx is written by the range with lo = 0. */
int pl_lifter_bwd_layers(const PLDesc* d, const float* x, const float* dy, int64_t B,
                         void* workspace, size_t workspace_bytes, float* dx,
                         float* flat_grads, int hi, int lo, void* stream);

/* One train_1.py:75-95 iteration body up to the optimiser in ONE call: model.train() forward
 * (baselineModel.py:87-102), MSELoss(mean) against target [B][out_dim] (train_1.py:94) and
 * loss.backward() (:95).  y [B][out_dim] and loss (1 float) are outputs; flat_grads is overwritten.
 * hi, lo as in pl_lifter_bwd_layers: the call with hi = L runs forward + loss first, then
 * backward over layers hi..lo; (L, 0) is the whole step.  Identical results to the separate calls. */
int pl_lifter_train_fwd_bwd(const PLDesc* d, const float* x, const float* target, int64_t B,
                            void* workspace, size_t workspace_bytes, uint64_t seed, uint64_t step,
                            float* y, float* loss, float* flat_grads, int hi, int lo, void* stream);

/* The WHOLE train_1.py:75-100 iteration body in one call: pl_lifter_train_fwd_bwd(.., L, 0, ..) and optimizer.step()
 * (train_1.py:39,89: torch.optim.AdamW) on d->params IN PLACE -- m, v: the exp_avg / exp_avg_sq arenas laid out like the
 * parameters; t the step number (>= 1); lr_dev / t_dev != NULL (graph replay): lr = *lr_dev and t = t + *t_dev, read on
 * the device.  At batches of <= 64 rows (the reference's own 64) whose hidden layers run as one launch each
 * (pl_lifter_step_carries_adamw = 1) the update has no launch of its own: each backward launch carries, on spare
 * workgroups, the slice of the arena whose gradients the launches before it finished and which nothing reads any more, and
 * one small launch updates the bottom of the arena (first layer, first residual Linear).  Otherwise: one pl_adamw_flat(_dev)
 * launch behind the backward pass.  Same element arithmetic as pl_adamw_flat either way.  The caller's persistent weight
 * planes (PLDesc.wplanes) are stale afterwards. */
/* Averaged (EMA) weights kept by the launch that updates the parameters: e has the parameter arena's layout and alignment
 * (16 bytes), and for every element the step updates, from the registers that hold the new parameter p_new,
 *     e = fmaf(p_new - e, omd, e)                  fp32, two roundings (the difference, the fused multiply-add)
 *     omd = (float)(1.0 - d_n), formed on the device in double: d_n = decay (warmup == 0), else min(decay, (1 + n) / (10 + n))
 *     n = t_taken - t0, the 1-based count of this update: t_taken = t + *t_dev - clip->skipped, the step number the bias
 *         corrections use; t0 = the taken-step count when the average was started (or loaded)
 * A step skipped by its clip record leaves e bitwise untouched, like p, m, v, and so does not count in n.
 * decay in [0, 1), e != NULL and 16-byte aligned, t0 >= 0: anything else is PL_EINVAL. */
typedef struct PLEma {
  float* e;
  float decay;
  int32_t warmup;
  int64_t t0;
} PLEma;
/* a <-> b over n floats in place (float4 where both are 16-byte aligned, scalar tail); the ranges must not overlap.
 * Evaluating with the averaged weights is this call over the parameter and EMA arenas, and once more to return. */
int pl_swap_f32(float* a, float* b, int64_t n, void* stream);
typedef struct PLAdamWStep {
  float* m;
  float* v;
  float lr;
  const float* lr_dev;
  float beta1, beta2, eps, weight_decay;
  int64_t t;
  const uint64_t* t_dev;
  const PLEma* ema; /* NULL, or the averaged weights of the whole arena: they follow inside the same launches (0.1.20) */
} PLAdamWStep;
int pl_lifter_step_carries_adamw(const PLDesc* d, int64_t B);
/* How many split-K sums of hidden layers' weight gradients a backward over layers hi .. lo (as in pl_lifter_bwd_layers) of B
 * rows carries inside the chained GEMM launch of the layer below instead of the range's closing reduce launch (hidden = 1024
 * at B = 4096: every hidden layer's but the lowest one's).  Same sums, same bits either way; < 0: a PLStatus. */
int pl_lifter_bwd_slab_rides(const PLDesc* d, int64_t B, int hi, int lo);
int pl_lifter_train_step(const PLDesc* d, const float* x, const float* target, int64_t B, void* workspace,
                         size_t workspace_bytes, uint64_t seed, uint64_t step, float* y, float* loss, float* flat_grads,
                         const PLAdamWStep* opt, void* stream);

/* ---- the train step's criterion (PARITY UNPINNED beyond MSELoss / L1Loss: the reference names only those two --
 * train_1.py:36-37, main.py:404-405, phase5_loop/losses.py:21, train_project.py:39 -- the oracle of the rest is torch) ----
 * pred, tgt [B][O] fp32, O = J * group (group = coordinates per joint: 3 lifter, 2 projector, 1 = no grouping), d = pred -
 * tgt, w_j = weights[j] (J device floats, NULL = all ones; they need not sum to anything), s = grad_scale.
 *
 *   kind        loss                                        d loss / d pred, element (b, j, g)
 *   mse         sum w_j d^2 / (B O)                         s 2 w_j d / (B O)
 *   l1          sum w_j |d| / (B O)                         s w_j sign(d) / (B O), 0 at d = 0
 *   smooth_l1   sum w_j rho(d) / (B O), rho = d^2 / (2 beta) if |d| < beta else |d| - beta / 2  (nn.SmoothL1Loss, beta > 0)
 *                                                           s w_j (d / beta or sign(d)) / (B O)
 *   mpjpe       sum_{b,j} w_j ||d_bj||_2 / (B J)            s w_j d / (||d_bj|| B J), 0 for the whole joint where ||d_bj|| = 0
 *
 * smooth_l1 with beta = 0 is rejected (use l1); Huber(delta) = delta * smooth_l1(beta = delta).  O % group != 0 is PL_ESHAPE,
 * and so is group > 4 on mpjpe.  Non-finite values come out where torch's do: l1's gradient at a NaN d is 0, smooth_l1's is
 * NaN, one NaN coordinate makes its whole joint's mpjpe gradient NaN.
 * The gradient in fp32, as computed (d = fl(pred - tgt); every product and quotient below rounded once):
 *   mse         (d * coef) [* w_j]                          coef = s * 2 / (float)(B O)
 *   l1          +-coef [* w_j], 0                           coef = s / (float)(B O)
 *   smooth_l1   |d| >= beta ? +-coef : d * cb  [* w_j]      cb = coef / beta
 *   mpjpe       d_g * (cw / r)                              coef = s / (float)(B J), cw = coef [* w_j], r = sqrtf(ss),
 *                                                           ss = d_0 d_0, then fmaf(d_g, d_g, ss) for g = 1 ..
 * All sums are taken in a fixed order without atomics: the same inputs give the same bits, eagerly or replayed.
 * A NULL criterion is plain MSE everywhere, and plain MSE runs the kernels and writes the bits it always did. */
typedef enum PLCriterionKind { PL_CRIT_MSE = 0, PL_CRIT_L1 = 1, PL_CRIT_SMOOTH_L1 = 2, PL_CRIT_MPJPE = 3 } PLCriterionKind;
typedef struct PLCriterion {
  int32_t kind;         /* a PLCriterionKind */
  int32_t group;        /* G >= 1 */
  float beta;           /* smooth_l1 only */
  const float* weights; /* device, O / group floats, or NULL */
} PLCriterion;
/* The criterion alone: loss (1 device float) and, dpred != NULL, its gradient [B][O], in one launch pair.  Any J.
 * scratch >= pl_pose_loss_scratch_bytes(B, O, crit).  pl_mse_fwd_bwd is the crit == NULL case of the same implementation.
 * (Here and for every *_scratch_bytes below: scratch may hold anything on entry, NaN bit patterns included, and nothing
 * is written outside the bytes the query answered -- UNINITIALISED MEMORY at pl_workspace_bytes.) */
size_t pl_pose_loss_scratch_bytes(int64_t B, int64_t O, const PLCriterion* crit);
int pl_pose_loss_fwd_bwd(const float* pred, const float* tgt, int64_t B, int64_t O, const PLCriterion* crit, float grad_scale,
                         float* dpred /* may be NULL */, float* loss, void* scratch, void* stream);
/* pl_lifter_train_fwd_bwd and pl_lifter_train_step with that criterion in place of MSELoss (crit == NULL: they ARE those
 * calls): the same (hi, lo) ranges, the same PLAdamWStep, the device step counter ticks at the same point, no launch more
 * than the MSE step on any route; identical results to pl_lifter_fwd_train, pl_pose_loss_fwd_bwd and pl_lifter_bwd in a row.
 * out_dim <= 64 routes (the small-batch layer kernels) take J <= 64 by construction. */
int pl_lifter_train_fwd_bwd_crit(const PLDesc* d, const float* x, const float* target, int64_t B, void* workspace,
                                 size_t workspace_bytes, uint64_t seed, uint64_t step, const PLCriterion* crit, float* y,
                                 float* loss, float* flat_grads, int hi, int lo, void* stream);
int pl_lifter_train_step_crit(const PLDesc* d, const float* x, const float* target, int64_t B, void* workspace,
                              size_t workspace_bytes, uint64_t seed, uint64_t step, const PLCriterion* crit, float* y,
                              float* loss, float* flat_grads, const PLAdamWStep* opt, void* stream);

/* ---- the skeleton terms of the criterion: bone lengths and left/right symmetry (PARITY UNPINNED: the reference has no
 * such loss; the oracle is torch autograd in fp64) ----
 * A skeleton on J joints (2 <= J <= 32) of G coordinates (G = the criterion's group, 2 or 3; J G = O) has K bones (c_k, p_k),
 * child and parent joint, 1 <= K <= 31, and S >= 0 symmetric pairs (k_L, k_R) of bone indices, S <= 16.  With the optional
 * inverse transform (sub, div, each [J G]: the numbers PoseTransform.invert uses) both tensors are first taken to raw
 * units, P = pred div + sub, T = tgt div + sub; without one P = pred, T = tgt.  lh_k = ||P_c - P_p||, l_k = ||T_c - T_p||,
 *
 *   L_bone = 1 / (B K) sum_{b,k} rho(lh_k - l_k)         L_sym = 1 / (B S) sum_{b,(kL,kR)} rho(lh_kL - lh_kR)   (prediction only)
 *   loss   = the base criterion + lambda_bone L_bone + lambda_sym L_sym,          rho(e) = |e| (l1) or e^2 (mse)
 *
 * d lh / d P_c = (P_c - P_p) / lh, 0 for the whole bone where lh == 0 (mpjpe's rule); rho'(0) = 0 for l1; the chain rule
 * through a transform multiplies by div per coordinate (a div == 0 column gets gradient 0); grad_scale multiplies everything.
 * The two lambdas are read by the kernel from device memory (term_weights): a weight schedule needs no re-capture of a graph,
 * and a lambda of 0 contributes exactly 0 to loss and gradient.  The terms cost one launch more per call; all sums are in a
 * fixed order without atomics.  Indices are the caller's contract: nothing here checks them against J or K,
 * nor that a bone joins two different joints and a pair two different bones.
 * In fp32, as computed (every operation rounded once; s = grad_scale):
 *   P = fl(fl(pred * div) + sub);  d_g = P_c,g - P_p,g;  ss = d_0 d_0, then fmaf(d_g, d_g, ss);  lh = sqrtf(ss)
 *   e = lh - l (pairs: lh_a - lh_b);  u_k = rho'(e) wb with wb = lambda_bone * cb, cb = s / (float)(B K): l1 +-wb or 0, mse
 *   e * (2 wb); then for each pair in order v = rho'(e) ws (ws = lambda_sym * cs, cs = s / (float)(B S)), u_a += v, u_b -= v
 *   r_k = lh_k == 0 ? 0 : u_k / lh_k;  x = d_g * r_k;  bones in order: g[c] += x [* div_c], g[p] -= x [* div_p];  dpred += g
 * Non-finite values come out where torch's do: a NaN coordinate of pred makes the loss NaN and the gradient NaN on every
 * coordinate of both joints of each bone that touches it, and leaves joints of clean bones and other poses alone.
 *
 * A criterion carries a skeleton as an extension of PLCriterion: set PL_CRIT_HAS_SKELETON in `kind` of a
 * PLSkeletonCriterion's base and pass &sc.base wherever a PLCriterion* goes.  Without the flag nothing past PLCriterion is
 * read, so every existing caller -- and a zero-initialised or NULL criterion -- behaves exactly as before.
 * PL_ESHAPE: joints * group != O, group not 2 or 3, joints, bones or pairs out of range; PL_EINVAL: a null table or
 * term_weights, an unknown rho, only one of sub / div. */
#define PL_CRIT_HAS_SKELETON 0x100
typedef struct PLSkeleton {
  int32_t joints, bones, pairs, rho;       /* rho: 0 = l1, 1 = mse */
  const int32_t* bone_child; const int32_t* bone_parent;       /* device, [bones] */
  const int32_t* pair_a; const int32_t* pair_b;                /* device, [pairs] bone indices, or NULL */
  const float* term_weights;                                   /* device, {lambda_bone, lambda_sym} */
  const float* sub; const float* div;                          /* device, [joints * group], or both NULL */
} PLSkeleton;
typedef struct PLSkeletonCriterion {
  PLCriterion base;                        /* base.kind = a PLCriterionKind | PL_CRIT_HAS_SKELETON */
  const PLSkeleton* skeleton;              /* NULL = none */
} PLSkeletonCriterion;
/* lengths [B][K] of poses [B][J][group] (raw units when the skeleton has a transform); reads only the bone table and
 * sub / div of *sk (pairs, rho and term_weights may be anything). */
int pl_bone_lengths(const float* poses, int64_t B, int32_t group, const PLSkeleton* sk, float* lengths, void* stream);
/* Test hooks.  pl_skeleton_terms_host: the same inline arithmetic compiled for the CPU -- every pointer, those inside *sk
 * included, is a host pointer.  *loss = lambda_bone L_bone + lambda_sym L_sym; dpred ([B][J G], may be NULL) is ADDED INTO;
 * lengths ([B][K], may be NULL) receives the prediction's bone lengths.
 * pl_skeleton_abi_bytes: sizeof of PLCriterion (0), PLSkeleton (1), PLSkeletonCriterion (2) as the library was compiled. */
int pl_skeleton_terms_host(const float* pred, const float* tgt, int64_t B, int32_t group, const PLSkeleton* sk,
                           float grad_scale, float* dpred, float* loss, float* lengths);
size_t pl_skeleton_abi_bytes(int which);

/* ---- per-pose joint weights ("row weights") of the criterion (PARITY UNPINNED: the oracle is torch's (W * elementwise).mean()) ----
 * rw [B][J] fp32 on the device, contiguous, J = O / group: the weight of joint j of pose b.  The effective weight is
 *   W_bj = rw[b][j]                    without per-joint weights (base.weights == NULL)
 *   W_bj = fl(w_j * rw[b][j])          with both: one fp32 product, formed once per element (mpjpe: per joint)
 * and W_bj stands wherever w_j stands in the table of PLCriterion above; nothing else changes.  The normaliser stays
 * 1 / (B O) (mpjpe: 1 / (B J)) whatever the weights sum to.  Weights multiply: a zero weight does not hide a NaN
 * (0 * NaN = NaN), as in torch.  There is no gradient with respect to rw.  The weight of flat element i of [B][O] is
 * rw[i / group]: same element map, same order of every sum, same number of partials and launches as the per-joint-weighted
 * criterion; rw[b][j] = w_j gives the bits of weights = w, and all-ones rw the bits of the unweighted criterion.
 *
 * Row weights ride behind PLCriterion as the skeleton does: set PL_CRIT_HAS_ROW_WEIGHTS in `kind` of sc.base and pass
 * &x.sc.base wherever a PLCriterion* goes (pl_pose_loss_fwd_bwd, pl_pose_loss_scratch_bytes, pl_lifter_train_fwd_bwd_crit,
 * pl_lifter_train_step_crit; under (hi, lo) ranges the weights are those of the call's own rows).  Without the flag nothing
 * past the skeleton extension is read.  Checked before anything is launched or counted:
 *   PL_EINVAL  the flag with a NULL row_weights; the flag together with PL_CRIT_HAS_SKELETON (the bone terms are not
 *              weighted per pose yet: the combination is not built)
 *   PL_ESHAPE  the flag with B O > INT32_MAX (the index arithmetic of the row-weight instantiations is 32-bit) */
#define PL_CRIT_HAS_ROW_WEIGHTS 0x200
typedef struct PLRowWeightsCriterion {
  PLSkeletonCriterion sc;                  /* sc.base.kind = a PLCriterionKind | PL_CRIT_HAS_ROW_WEIGHTS; sc.skeleton unread without its flag */
  const float* row_weights;                /* device, [B][O / group] */
} PLRowWeightsCriterion;
/* Test hook: sizeof of PLCriterion (0), PLSkeleton (1), PLSkeletonCriterion (2), PLRowWeightsCriterion (3) as the library was
 * compiled, 0 for anything else.  (pl_skeleton_abi_bytes keeps answering 0 for 3, as its callers pin.) */
size_t pl_criterion_abi_bytes(int which);

/* The 3-D head forward on NHWC logits [B][H][W][J*64] (depth_dim 64, the conv path's layout): same
 * coords [B*J][3] and stats [B*J][5] as pl_softargmax_fwd(ncoord 3, centred 1).  Model.py:94-133. */
int pl_softargmax3d_nhwc_fwd(const float* logits, int64_t B, int64_t J, int64_t H, int64_t W,
                             float* coords, float* stats, void* stream);
/* Backward of pl_softargmax3d_nhwc_fwd: dlogits [B][H*W][J*64] from the saved logits, the forward's stats [B*J][5]
 * and the coordinate gradients gcoords [B*J][3]; one streaming pass (4 B read + 4 B written per voxel), so a
 * training step needs no NHWC <-> NCHW pass around the head (phase4_joined/Model.py:94-133 under autograd). */
int pl_softargmax3d_nhwc_bwd(const float* logits, const float* stats, const float* gcoords, int64_t B, int64_t J,
                             int64_t H, int64_t W, float* dlogits, void* stream);

/* ---- convolution path (first slice: forward) ------------------------ */
/* nn.Conv2d forward in NHWC with the Bottleneck's eval-mode epilogue folded in: phase4_joined/Resnet.py:51-95
 * (conv1/2/3 + bn + relu + residual), :112-118 (7x7 stem), :151-158 (downsample), phase4_joined/Model.py:66-69
 * (final 1x1 conv with bias).
 *   v = sum_{kh,kw,ci} x[b][oh*stride - pad + kh][ow*stride - pad + kw][ci] * w[co][kh][kw][ci]  (+ bias[co])
 *   v = v * scale[co] + shift[co]          (BatchNorm2d on running statistics, folded; or NULL)
 *   relu 1: v = max(v, 0), then v += resid;   relu 2: v += resid, then max(v, 0);   relu 0: v += resid
 * x [B][H][W][Cin], w [Cout][KH][KW][Cin] (OHWI), resid / y [B][Ho][Wo][Cout].
 * Cin % 32 == 0: implicit GEMM on the PL_BF16X6 pipeline (fp32-grade products, no im2col buffer; ragged last
 * row / column tiles are clamped and masked); 1x1 stride 1: a plain GEMM; anything else (the stem with Cin = 3):
 * explicit im2col into `scratch` (>= pl_conv2d_nhwc_scratch_bytes, 0 for the others).
 * arith: PL_BF16X6 (fp32-grade) or PL_BF16 (operands rounded to bf16 while staged, one MFMA product: the
 * throughput mode; storage stays fp32). */
size_t pl_conv2d_nhwc_scratch_bytes(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH,
                                    int KW, int stride, int pad);
/* the same knowing the epilogue of the call (the 7x7 / Cin 3 stem needs no scratch unless it carries a bias, a residual
 * or relu == 2; the plain query answers for that worst case) */
size_t pl_conv2d_nhwc_scratch_bytes_ex(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH,
                                       int KW, int stride, int pad, int has_bias, int has_resid, int relu);
int pl_conv2d_nhwc_fwd(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* w,
                       int64_t Cout, int KH, int KW, int stride, int pad, const float* scale,
                       const float* shift, const float* bias, int relu, const float* resid, float* y,
                       int arith, void* scratch, size_t scratch_bytes, void* stream);

/* Weight gradient of the same convolution (autograd of nn.Conv2d, phase4_joined/train.py:80 loss.backward()):
 * dw [Cout][KH][KW][Cin] = sum_{b,oh,ow} dy[b][oh][ow][co] * x[b][oh*stride - pad + kh][ow*stride - pad + kw][ci],
 * the TN GEMM over pixels with x gathered on the fly, split over the pixels so that it fills the chip (fixed-order
 * slab combine, no float atomics).  Cout and Cin even, Wo % 8 == 0 and B*Ho*Wo % 32 == 0 take the gathered kernel
 * (ragged tiles clamped and masked); other shapes an explicit im2col + the generic GEMM in scratch; the 7x7 / Cin = 3
 * stem its own exact-fp32 kernel.  arith: PL_BF16X6 (fp32-grade) or PL_BF16 (operands rounded to bf16 while staged,
 * fp32 accumulate and output).  The input gradient needs no kernel of its own: stride 1 = pl_conv2d_nhwc_fwd on dy with
 * the flipped, transposed filter; stride 2 = pl_deconv4x4s2_nhwc_fwd (conv.py conv2d_nhwc_dgrad). */
size_t pl_conv2d_nhwc_wgrad_scratch_bytes(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                          int KH, int KW, int stride, int pad);
int pl_conv2d_nhwc_wgrad(const float* x, int64_t B, int64_t H, int64_t W, int64_t Cin, const float* dy,
                         int64_t Cout, int KH, int KW, int stride, int pad, float* dw, int arith, void* scratch,
                         size_t scratch_bytes, void* stream);

/* Training-mode BatchNorm (+ ReLU) over the rows of a [rows][C] fp32 matrix: nn.BatchNorm2d on an NHWC feature map
 * ([B*H*W][C]; phase4_joined/Resnet.py:56-63, Model.py:52-58) -- or BatchNorm1d -- with batch statistics, running
 * statistics updated as torch does (momentum, unbiased variance, num_batches += 1).  C % 4 == 0, rows >= 2.
 *   fwd: y = [relu](gamma * (z - mean) * rstd + beta); bits [rows][4*ceil(C/256)] 64-bit words (the layout of
 *        pl_workspace_view which = 2): 1 where the output passed the ReLU (all ones without it); mean, rstd [C] saved.
 *   bwd: dz, dgamma [C], dbeta [C] from dy and what fwd saved.
 * scratch >= pl_bn_train_scratch_bytes(rows, C) for both. */
size_t pl_bn_train_scratch_bytes(int64_t rows, int64_t C);
int pl_bn_train_fwd(const float* z, int64_t rows, int64_t C, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, int64_t* batches, int relu,
                    float* y, uint64_t* bits, float* mean, float* rstd, void* scratch, void* stream);
int pl_bn_train_bwd(const float* dy, const uint64_t* bits, const float* z, const float* mean, const float* rstd,
                    const float* gamma, int64_t rows, int64_t C, float* dz, float* dgamma, float* dbeta,
                    void* scratch, void* stream);
/* The residual join of a Bottleneck in training mode (Resnet.py:90-91): out = relu(a + b) and its bitmap;
 * backward: both inputs receive pl_mask_by_bits(g). */
int pl_add_relu_fwd(const float* a, const float* b, int64_t rows, int64_t C, float* out, uint64_t* bits, void* stream);
int pl_mask_by_bits(const float* g, const uint64_t* bits, int64_t rows, int64_t C, float* dx, void* stream);

/* The same building blocks writing GEMM OPERAND PLANES (the conv path's 1x1 convolutions on the planes GEMM, as the
 * lifter's 1024-wide Linears: the kernel that produces a tensor also writes it as 16-bit planes, the GEMM stages them by
 * LDS-DMA).  planes of an n-element tensor: planes_mode PL_F16X3 -> [2][n] fp16 (h = fp16(S x), l = fp16((S x - h) 2048)),
 * PL_BF16 -> [n] bf16; 16-byte aligned, n % 8 == 0; NULL = none.  Replaces the same reference code as the plain forms.
 *   pl_planes_split     : planes of an fp32 tensor with the static scale S (weights: 16; conv-path activations:
 *                         pl_conv_act_plane_scale() = 1/64 -- eval-mode maps of an unnormalised network reach 1e5)
 *   pl_bn_train_fwd_ex  : y may be NULL when only the planes are wanted (S = pl_conv_act_plane_scale()); gemm_stat (optional): the batch statistics
 *                         as the producing GEMM's epilogue left them -- [2][pl_gemm_stat_groups(rows)][C]: per 64-row group
 *                         the column sums, then the sums of squares about the group mean -- instead of a pass over z
 *                         join (optional, relu != 0): y = relu(bn(z) + join) in the same pass -- the Bottleneck's bn3 and
 *                         residual join (Resnet.py:81-91); bits then is the join's ReLU bitmap
 *   pl_bn_train_bwd_ex  : dz may be NULL; PL_F16X3 planes hold S dz with S a power of two chosen on the device from a range
 *                         bound of dz; dz_scale (device, 2 floats) receives {S, 1/S} -- pass dz_scale + 1 as dyn_inv below
 *   pl_add_relu_fwd_ex  : out (fp32, the next join reads it) AND its planes (S = pl_conv_act_plane_scale())
 *   pl_mask_add_by_bits : dx = (g + g2) masked (g2 may be NULL): the join's backward with the gradient sum folded in */
float pl_conv_act_plane_scale(void);   /* S of every activation-plane output of the conv-path entries below (1/64) */
int pl_planes_split(const float* x, int64_t n, int planes_mode, float scale, void* planes, void* stream);
/* The same from a strided 4-D view of the source (a convolution weight in the layout its GEMM wants -- OIHW -> OHWI, the
 * transpose, the spatial flip of conv.py's data gradients -- straight from the nn.Conv2d parameter, one launch): element
 * (i0,i1,i2,i3) of the contiguous result is x[i0 s0 + i1 s1 + i2 s2 + i3 s3]; x points at the view's first element, strides are
 * in elements and signed (a flipped axis has a negative one); dims[3] % 4 == 0. */
int pl_planes_split_strided(const float* x, const int64_t* dims, const int64_t* strides, int planes_mode, float scale,
                            void* planes, void* stream);
int pl_bn_train_fwd_ex(const float* z, int64_t rows, int64_t C, const float* gamma, const float* beta, float eps,
                       float momentum, float* running_mean, float* running_var, int64_t* batches, int relu,
                       float* y, uint64_t* bits, float* mean, float* rstd, void* scratch, void* y_planes,
                       int planes_mode, const float* gemm_stat, const float* join, void* stream);
int pl_bn_train_bwd_ex(const float* dy, const uint64_t* bits, const float* z, const float* mean, const float* rstd,
                       const float* gamma, int64_t rows, int64_t C, float* dz, float* dgamma, float* dbeta,
                       void* scratch, void* dz_planes, int planes_mode, float* dz_scale, void* stream);
int pl_add_relu_fwd_ex(const float* a, const float* b, int64_t rows, int64_t C, float* out, uint64_t* bits,
                       void* out_planes, int planes_mode, void* stream);
int pl_mask_add_by_bits(const float* g, const float* g2, const uint64_t* bits, int64_t rows, int64_t C, float* dx,
                        void* stream);
/* Backward of bn3 + residual join in one go (Resnet.py:81-91 under autograd): dx = (g + g2) where the join's bitmap is set
 * (g2 may be NULL) -- the identity's gradient and bn3's dy -- written by the pass that also takes BatchNorm-backward's column
 * sums; then the finalize and dz as pl_bn_train_bwd_ex (same scratch, same dz / dz_planes / dz_scale meaning).  C >= 256. */
int pl_bn_join_bwd(const float* g, const float* g2, const uint64_t* bits, const float* z, const float* mean,
                   const float* rstd, const float* gamma, int64_t rows, int64_t C, float* dx, float* dz, float* dgamma,
                   float* dbeta, void* scratch, void* dz_planes, int planes_mode, float* dz_scale, void* stream);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1)  phase4_joined/Resnet.py:119.  x [B][H][W][C], C % 4 == 0;
 * y [B][(H-1)/2+1][(W-1)/2+1][C]. */
int pl_maxpool3x3s2_nhwc(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y, void* stream);
/* its backward: dx [B][H][W][C] from the forward input x and dy [B][Ho][Wo][C]; a window's gradient goes to its first
 * maximum in (kh, kw) order, recomputed from x (no index tensor, no atomics). */
int pl_maxpool3x3s2_nhwc_bwd(const float* x, const float* dy, int64_t B, int64_t H, int64_t W, int64_t C,
                             float* dx, void* stream);
/* The training-mode pair (what autograd's MaxPool2d keeps is an index tensor too): the forward also writes, one
 * byte per output element, the tap kh*3 + kw of the first maximum; the backward reads those bytes and dy only. */
int pl_maxpool3x3s2_nhwc_idx(const float* x, int64_t B, int64_t H, int64_t W, int64_t C, float* y,
                             unsigned char* idx, void* stream);
int pl_maxpool3x3s2_nhwc_bwd_idx(const unsigned char* idx, const float* dy, int64_t B, int64_t H, int64_t W,
                                 int64_t C, float* dx, void* stream);
/* y [B][2Hi][2Wi][C]: x on the even pixels, zero elsewhere -- the input gradient of a 1x1 stride-2 convolution
 * (the downsample branches, Resnet.py:151-158) is dy W (a GEMM) placed this way. */
int pl_upsample2x_zero_nhwc(const float* x, int64_t B, int64_t Hi, int64_t Wi, int64_t C, float* y, void* stream);
/* out[c] = sum_r X[r][c] (fixed order): the bias gradient of the final 1x1 convolution (Model.py:66-69). */
size_t pl_colsum_scratch_bytes(int64_t rows, int64_t cols);
int pl_colsum(const float* X, int64_t rows, int64_t cols, float* out, void* scratch, void* stream);

/* nn.ConvTranspose2d(kernel_size=4, stride=2, padding=1, bias=False) + folded BatchNorm2d + ReLU
 * phase4_joined/Model.py:47-63: x [B][Hi][Wi][Cin] -> y [B][2Hi][2Wi][Cout].  Each output parity
 * (oh&1, ow&1) is a 2x2-tap convolution over the input: four implicit GEMMs at the INPUT resolution (no
 * zero insertion, no wasted MACs) and one interleave pass.  w_sub [4][Cout][2][2][Cin]: parity
 * (ph, pw) = index ph*2 + pw, tap (th, tw) = weight[ci][co][kh][kw] with kh = (ph ? 2 : 3) - 2*th, kw
 * likewise.  Cin % 32 == 0.  scratch >= ..._scratch_bytes. */
size_t pl_deconv4x4s2_nhwc_scratch_bytes(int64_t B, int64_t Hi, int64_t Wi, int64_t Cout);
int pl_deconv4x4s2_nhwc_fwd(const float* x, int64_t B, int64_t Hi, int64_t Wi, int64_t Cin,
                            const float* w_sub, int64_t Cout, const float* scale, const float* shift,
                            int relu, float* y, int arith, void* scratch, size_t scratch_bytes, void* stream);

/* [B][P][C] -> [B][C][P]: the head's NHWC logits to the [B][J*D][H*W] layout of pl_softargmax_fwd. */
int pl_nhwc_to_nchw(const float* in, int64_t B, int64_t P, int64_t C, float* out, void* stream);

/* ---- batch feed ------------------------------------------------------------------- */
/* One batch of the DataLoader path (train_1.py:26-31,75-81: shuffle, collate, .float(), .to(device))
 * from tables resident in HBM: oa[i] = a[idx[i]] (wa floats per row, the (17,2) keypoints),
 * ob[i] = b[idx[i]] (wb floats, the (17,3) targets), i < n.  idx: device int64, every value in
 * [0, table_rows) (the caller's permutation; not checked on the device). */
int pl_gather_rows2(const float* a, int64_t wa, const float* b, int64_t wb, const int64_t* idx,
                    int64_t n, int64_t table_rows, float* oa, float* ob, void* stream);

/* The same batch with seeded train-time augmentation applied where the rows are read (csrc/pose_augment.h has the
 * definition; the reference leaves it commented out, per sample, at phase3_direct/my_HybrIK/H36_dataset.py:98-117 and
 * phase1_lifting/train_1.py:83-84).  Poses are 17 joints: a [rows][34] = (17,2), b [rows][51] = (17,3).
 *   2-D: flip (flip_pose's joint swap, x -> flip_offset - x), rotate about (cx, cy), scale about (cx, cy), translate, add
 *        Gaussian noise;   3-D: flip (x -> -x), rotate (x, y) by the same angle; z untouched.
 * Image x right / y down, the 3-D target camera-frame and root-relative; scale and translation leave it alone (weak
 * perspective).  A parameter of 0 switches its stage off exactly: the all-zero PLPoseAug writes pl_gather_rows2's bits.
 * Every draw of a pose is a Philox4x32-10 function of (seed, epoch, row_id) -- never of the batch size, the position in
 * the batch or the rank -- on a key tagged apart from the dropout stream. */
typedef struct PLPoseAug {
  float p_flip;       /* probability of the horizontal flip: <= 0 never, >= 1 always */
  float flip_offset;  /* 2-D flip is x -> flip_offset - x: 1 for image-normalised x (utils.py:391); augment raw poses and standardise behind it (pl_pose_augment_gather_t) */
  float max_rot;      /* rotation angle uniform in [-max_rot, max_rot) radians */
  float scale_range;  /* 2-D scale uniform in [1 - scale_range, 1 + scale_range); < 1 */
  float max_shift;    /* 2-D translation (tx, ty), each uniform in [-max_shift, max_shift) */
  float jitter_sigma; /* std of the Gaussian noise on every 2-D coordinate (train_1.py:84 used 0.05) */
  float cx, cy;       /* centre of rotation and scale in 2-D */
  uint64_t seed;
} PLPoseAug;
/* oa[k], ob[k] = augment(a[s], b[s]; draws of row_id[k]), s = src_idx[k], or k when src_idx is NULL (an already gathered
 * batch: n <= table_rows), k < n.  src_idx, row_id: int64; an s outside [0, table_rows) reads nothing and gives a NaN
 * pose on the device, PL_EINVAL on the host.  The outputs may overlap neither each other nor a source.  Negative or
 * non-finite parameters and scale_range >= 1 are PL_EINVAL.  One launch on `stream`; no allocation, no synchronisation.
 * pl_pose_augment_host: the same inline text compiled for the CPU, on host pointers (a test hook). */
int pl_pose_augment_gather(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                           int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch, void* stream);
int pl_pose_augment_host(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                         int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch);

/* The per-pose joint weights (PLRowWeightsCriterion) of the same batch: out[k][j] = w[s][flipped_k ? flip_src_joint(j) : j],
 * s = src_idx[k], or k when src_idx is NULL; w [table_rows][J], out [n][J].  flipped_k is the flip bit
 * pl_pose_augment_gather forms for (aug->seed, epoch, row_id[k]) -- the same functions of csrc/pose_augment.h -- so the
 * weights follow the joints through the left/right swap; no other stage moves a joint.  aug == NULL or p_flip <= 0: a plain
 * gather, any J >= 1 (row_id may then be NULL); otherwise J = 17, else PL_ESHAPE.  An s outside [0, table_rows) writes a NaN
 * row on the device and is PL_EINVAL on the host.  One small launch; pl_row_weights_gather_host: the same inline text on
 * host pointers (a test hook). */
int pl_row_weights_gather(const float* w, const int64_t* src_idx, const int64_t* row_id, int64_t n, int64_t table_rows,
                          int64_t J, float* out, const PLPoseAug* aug, uint64_t epoch, void* stream);
int pl_row_weights_gather_host(const float* w, const int64_t* src_idx, const int64_t* row_id, int64_t n, int64_t table_rows,
                               int64_t J, float* out, const PLPoseAug* aug, uint64_t epoch);

/* pl_pose_augment_gather with two nullable per-column transforms (pose tables, below), applied to each output element
 * AFTER the augmentation: oa's 34 columns become (v - sub_a[c]) / div_a[c], ob's 51 (v - sub_b[c]) / div_b[c]; a column
 * with div == 0 becomes 0.  Tables stay raw, so flip, rotation, scale, shift and jitter keep their image units, and the
 * batch leaves standardised in the same launch.  A transform is a (sub, div) pair of device (host: _host_t) arrays; with
 * both pairs NULL the call is pl_pose_augment_gather, the same kernel instantiation.  The NaN pose of a bad source index goes
 * through the transform like any value. */
int pl_pose_augment_gather_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                             int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                             const float* sub_a, const float* div_a, const float* sub_b, const float* div_b, void* stream);
int pl_pose_augment_host_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                           int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                           const float* sub_a, const float* div_a, const float* sub_b, const float* div_b);

/* ---- pose tables: prepare, statistics, the per-column transform (csrc/pose_table.h has the definitions) ---------------
 * What the reference does per frame and per joint in Python before training and undoes before it measures
 * (phase3_direct/my_HybrIK/H36_dataset.py:303-379 read_data, :205-300 process_data; phase1_lifting/main.py:473-474).
 *
 * pl_pose_prepare: raw [N][Jsrc][D] fp32 (D in {2, 3}, 1 <= Jsrc <= 64) -> out [N][J][D] (1 <= J <= 32), stages in the
 * reference's order, a stage that is off not run at all:
 *   pick        out[n][j] = raw[n][pick[j]]; pick: HOST int32 [J] or NULL (then J == Jsrc).  An index outside [0, Jsrc)
 *               is PL_ESHAPE and nothing is launched.                                                      (:335)
 *   camera view D = 3, on when cameras != NULL (cam_id then too; with D = 2: PL_ESHAPE).  cameras [C][7] fp64 =
 *               (t0, t1, t2, w, x, y, z): translation in the poses' units (the caller divides millimetres by 1000) and
 *               the orientation quaternion; cam_id [N] int32.  v = q (0, (double)p - t) q*, both Hamilton products term
 *               by term in utils.py:328-335's order, fp64, no contraction, rounded to fp32 once.  A cam_id outside
 *               [0, C) reads no camera and makes every element of that row NaN.                            (:357-360)
 *   zero_centre joints 1..J-1 minus joint 0 in fp32; joint 0 becomes +0.                                  (:209-211, :288-289)
 * out may not overlap raw.  One launch.
 *
 * pl_pose_stats: x [N][W] fp32, W = J D <= 96 -> out [4][W] fp64 on the device: mean, std (population, two passes about
 * the mean: sqrt(sum (x - mean)^2 / N), :215-222), min, max.  fp64 accumulation, no atomics, four launches, nothing on
 * the host in between; every sum in an order that depends on (N, W) alone (chunks of pl_pose_stats_chunk_rows() rows),
 * so the same table gives the same bits on every run and stream.  A NaN makes all four values of its column NaN and no
 * other column's; +inf gives mean = max = inf, std = NaN (numpy's answers).  A constant column (min == max) has mean =
 * that value exactly and std = +0.  scratch >= pl_pose_stats_scratch_bytes(N, W), 8-byte aligned.
 *
 * pl_pose_affine: x [N][W] -> y [N][W], per column (sub[c], div[c]) fp32.  invert = 0: y = (x - sub) / div, a correctly
 * rounded division (:272, :283; normalisation :269, :279-280 are the same form).  invert != 0: x = y div + sub, two
 * roundings (main.py:473-474).  A column with div == 0 applies to 0 and inverts to sub -- the zeroed root joint and any
 * constant column; the reference keeps 0/0 = NaN there.  y == x (in place) is allowed, any other overlap is PL_EINVAL.
 *
 * The _host forms run the same inline text on host pointers (test hooks). */
int pl_pose_prepare(const float* raw, int64_t N, int64_t Jsrc, int64_t D, const int32_t* pick_or_null, int64_t J,
                    const int32_t* cam_id_or_null, const double* cameras_or_null, int64_t C, int zero_centre, float* out,
                    void* stream);
int pl_pose_prepare_host(const float* raw, int64_t N, int64_t Jsrc, int64_t D, const int32_t* pick_or_null, int64_t J,
                         const int32_t* cam_id_or_null, const double* cameras_or_null, int64_t C, int zero_centre, float* out);
int64_t pl_pose_stats_chunk_rows(void);
size_t pl_pose_stats_scratch_bytes(int64_t N, int64_t W);
int pl_pose_stats(const float* x, int64_t N, int64_t W, double* out /* [4][W] */, void* scratch, void* stream);
int pl_pose_stats_host(const float* x, int64_t N, int64_t W, double* out);
int pl_pose_affine(const float* x, int64_t N, int64_t W, const float* sub, const float* div, int invert, float* y, void* stream);
int pl_pose_affine_host(const float* x, int64_t N, int64_t W, const float* sub, const float* div, int invert, float* y);

/* ---- video tracks: detector keypoints to filtered 3-D poses (csrc/track.h has the definitions) -----------------------
 * The reference keeps one [17][3] (x, y, confidence) row per video frame, COCO-17 mapped to the H36M-17 layout, all zeros
 * where nothing was detected (phase1_lifting/video2keypoints.py:14-57, :83-98).  PARITY UNPINNED: it remaps the two
 * coordinate columns only and leaves the confidence column in COCO order (:94-95); here a joint's confidence follows it.
 * Every entry is ONE launch on `stream`, allocates nothing and synchronises nothing; the _host forms run the same inline
 * text on host pointers (test hooks).  seq_ids_or_null [T] int32: the frames of one video are contiguous; frame s is in frame
 * t's sequence when every frame from t to s carries the same id; NULL = one sequence.  Nothing reads across a boundary.
 * T outside [1, 8 INT32_MAX] is PL_ESHAPE; a null required pointer, outputs that overlap an input or each other: PL_EINVAL.
 *
 * pl_track_remap: det [T][17][3] -> out [T][17][3] in the H36M-17 layout.  layout PL_TRACK_COCO17: the arithmetic of
 *   coco2h36m in fp32 in its order (a midpoint is (a + b) * 0.5f, joint 7 from the computed joints 0 and 8); a derived
 *   joint's confidence is the minimum of its sources' (a NaN wins).  PL_TRACK_H36M17: a copy.
 * pl_track_prepare: remap, scale (x / div_w, y / div_h: correctly rounded), validity (conf >= conf_thr, both coordinates
 *   finite) and gap fill, max_gap G in 0..64, searched at most G frames each way inside the sequence:
 *     state 0 valid         xy = the scaled detection                                   w = conf
 *     state 1 interpolated  a < t < b found, b - a - 1 <= G: x_a + (x_b - x_a) * ((float)(t - a) / (float)(b - a))
 *                                                                                       w = fill_conf * min(conf_a, conf_b)
 *     state 2 held          one side found, the other side's search left the sequence  w = fill_conf * conf_side
 *     state 3 lost          the detection's own scaled value where finite, else 0       w = 0
 *   xy [T][17][2], w [T][17] fp32, state [T][17] uint8.  PL_EINVAL: div not positive and finite, conf_thr NaN, fill_conf
 *   negative or not finite, max_gap outside 0..64, an unknown layout.
 * pl_track_filter: x [T][J][D] (D in {2, 3}, J <= 32), w_or_null [T][J], taps [K] ON THE HOST, K odd and <= 65:
 *     y[t][j][:] = (sum_k taps[k] w[s][j] x[s][j][:]) / (sum_k taps[k] w[s][j]),  s = t + k - K/2 inside t's sequence,
 *   fp32 in increasing k, one correctly rounded division per element; a sample with w == 0 is skipped, NULL w is weight 1, a
 *   denominator that is not positive gives y = x[t].  PL_EINVAL: K even or outside 1..65, a tap negative or not finite;
 *   PL_ESHAPE: J or D out of range.  A workgroup stages pl_track_filter_tile_frames(J, D, K) frames plus halo in LDS.
 * pl_track_velocity_errors: pred, tgt [T][J][3] -> out [T][J]: order 1 ||(p[t] - p[t-1]) - (g[t] - g[t-1])||, order 2 the
 *   same with q[t+1] - 2 q[t] + q[t-1]; count [T] uint8 = 1 where the stencil lies inside t's sequence, out = 0 elsewhere.
 *   (sub, div) [3 J] or both NULL: the poses are taken back first as pl_pose_errors_t does. */
enum { PL_TRACK_COCO17 = 0, PL_TRACK_H36M17 = 1 };
int pl_track_remap(const float* det, int64_t T, int layout, float* out, void* stream);
int pl_track_remap_host(const float* det, int64_t T, int layout, float* out);
int pl_track_prepare(const float* det, int64_t T, int layout, float div_w, float div_h, float conf_thr, int max_gap,
                     float fill_conf, const int32_t* seq_ids_or_null, float* xy, float* w, uint8_t* state, void* stream);
int pl_track_prepare_host(const float* det, int64_t T, int layout, float div_w, float div_h, float conf_thr, int max_gap,
                          float fill_conf, const int32_t* seq_ids_or_null, float* xy, float* w, uint8_t* state);
int pl_track_filter_tile_frames(int64_t J, int64_t D, int K);
int pl_track_filter(const float* x, int64_t T, int64_t J, int64_t D, const float* w_or_null, const int32_t* seq_ids_or_null,
                    const float* taps, int K, float* y, void* stream);
int pl_track_filter_host(const float* x, int64_t T, int64_t J, int64_t D, const float* w_or_null,
                         const int32_t* seq_ids_or_null, const float* taps, int K, float* y);
int pl_track_velocity_errors(const float* pred, const float* tgt, int64_t T, int64_t J, const int32_t* seq_ids_or_null,
                             int order, const float* sub_or_null, const float* div_or_null, float* out, uint8_t* count,
                             void* stream);
int pl_track_velocity_errors_host(const float* pred, const float* tgt, int64_t T, int64_t J, const int32_t* seq_ids_or_null,
                                  int order, const float* sub_or_null, const float* div_or_null, float* out, uint8_t* count);

/* ---- cameras: projection, reprojection loss, root translation (csrc/camera.h has the definitions) ---------------------
 * The reference carries the Human3.6M intrinsics (phase3_direct/my_HybrIK/utils.py:131-172) and never projects with them
 * (Model.py:185-189 is commented out).  PARITY UNPINNED: the distortion model is the one in common use for these coefficients.
 * Shared arguments: X [B][J][3] camera-frame (or, with t, root-relative) poses, J <= 32; cams [C][9] fp32 rows
 * (fx, fy, cx, cy, k1, k2, k3, p1, p2); cam_ids_or_null [B] int32 (NULL: every pose uses row 0; an id outside [0, C) reads no
 * row: every value of its pose that depends on the camera is NaN); t_or_null [B][3] added to every joint of its pose; (sub, div) [J][3] or both NULL:
 * X is taken to raw units first, q = x div + sub, as pl_pose_errors_t does, and gradients are chained through div.
 *   x = X/Z, y = Y/Z, r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)), tan = p1 x + p2 y,
 *   u = fx (x (rad + tan) + p1 r2) + cx,  v = fy (y (rad + tan) + p2 r2) + cy
 * in fp32, every operation rounded by itself, divisions and square roots correctly rounded, no clamp and no special case for
 * Z <= 0.  Every entry enqueues on `stream` (the loss: two launches, the others one), allocates nothing and synchronises
 * nothing; the _host forms run the same inline text on host pointers (test hooks) and give the same bits.  No tensor needs
 * more than 4-byte alignment (the loss's scratch, fp64 partial sums: 8).  PL_ESHAPE: B outside [1, INT32_MAX], J outside [1, 32], C < 1; PL_EINVAL: a null required
 * pointer, sub without div, outputs that overlap an input or each other, and what each entry names below.
 *
 * pl_camera_project: uv [B][J][2].
 * pl_camera_project_bwd: duv [B][J][2] -> dX [B][J][3] by the analytic Jacobian, and dT_or_null [B][3] = the sum of the pose's
 *   joint gradients in joint order (PL_EINVAL: dT without t).
 * pl_camera_reproj_errors: err [B][J] = sqrtf(du du + dv dv), du = (u - target_u) / div_w, dv = (v - target_v) / div_h against
 *   target [B][J][2]; div positive and finite (else PL_EINVAL), (1, 1) for pixels.
 * pl_camera_reproj_loss_fwd_bwd: loss[0] and its gradient times grad_scale.  kind PL_REPROJ_L1: mean of |du| + |dv| over
 *   B J 2 elements; PL_REPROJ_MSE: of du du + dv dv over B J 2; PL_REPROJ_L2: of the pixel distance over B J.
 *   weights_or_null [B][J] MULTIPLY a joint's value (0 * NaN = NaN: a zero weight hides no NaN); the normaliser stays the
 *   element count.  dX_or_null (NULL: the value alone), dT_or_null (needs t and dX).  scratch: at least
 *   pl_camera_reproj_loss_scratch_bytes(B, J) bytes, 8-byte aligned, written before it is read.  The sums have a fixed order,
 *   a function of (B, J) alone (camera.h).
 * pl_camera_fit_translation: per pose the t [B][3] that places the root-relative X in front of its camera so that it
 *   reprojects onto target [B][J][2] (pixels), and rms [B], the weighted RMS reprojection error after the last step.  A joint
 *   takes part iff its weight is > 0 (weights SELECT here; NULL: all).  A linear initialisation that ignores distortion, then
 *   `iters` (0..8, else PL_EINVAL) Gauss-Newton steps on the distorted model: a fixed count, no convergence test.  The 3 x 3
 *   systems are accumulated and solved in fp64.  Fewer than two joints taking part, or a system whose determinant is not
 *   positive (camera.h: kDetFloor): t and rms of that pose are NaN and no other pose is touched. */
enum { PL_REPROJ_L1 = 0, PL_REPROJ_MSE = 1, PL_REPROJ_L2 = 2 };
int pl_camera_project(const float* X, int64_t B, int64_t J, const float* cams, int64_t C, const int32_t* cam_ids_or_null,
                      const float* t_or_null, const float* sub_or_null, const float* div_or_null, float* uv, void* stream);
int pl_camera_project_host(const float* X, int64_t B, int64_t J, const float* cams, int64_t C, const int32_t* cam_ids_or_null,
                           const float* t_or_null, const float* sub_or_null, const float* div_or_null, float* uv);
int pl_camera_project_bwd(const float* X, const float* duv, int64_t B, int64_t J, const float* cams, int64_t C,
                          const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                          const float* div_or_null, float* dX, float* dT_or_null, void* stream);
int pl_camera_project_bwd_host(const float* X, const float* duv, int64_t B, int64_t J, const float* cams, int64_t C,
                               const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                               const float* div_or_null, float* dX, float* dT_or_null);
int pl_camera_reproj_errors(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                            const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                            const float* div_or_null, float div_w, float div_h, float* err, void* stream);
int pl_camera_reproj_errors_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                 const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                 const float* div_or_null, float div_w, float div_h, float* err);
size_t pl_camera_reproj_loss_scratch_bytes(int64_t B, int64_t J);
int pl_camera_reproj_loss_fwd_bwd(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                  const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                  const float* div_or_null, const float* weights_or_null, int kind, float div_w, float div_h,
                                  float grad_scale, float* dX_or_null, float* dT_or_null, float* loss, void* scratch,
                                  void* stream);
int pl_camera_reproj_loss_fwd_bwd_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                       const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                       const float* div_or_null, const float* weights_or_null, int kind, float div_w,
                                       float div_h, float grad_scale, float* dX_or_null, float* dT_or_null, float* loss,
                                       void* scratch);
int pl_camera_fit_translation(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                              const int32_t* cam_ids_or_null, const float* weights_or_null, const float* sub_or_null,
                              const float* div_or_null, int iters, float* t, float* rms, void* stream);
int pl_camera_fit_translation_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                   const int32_t* cam_ids_or_null, const float* weights_or_null, const float* sub_or_null,
                                   const float* div_or_null, int iters, float* t, float* rms);

/* The frames of the same rows, gathered, resized, normalised and augmented in one launch (csrc/frame_warp.h has the
 * definition; the reference resizes per sample on the host, H36_dataset.py:129-131 `cv2.resize(frame,(256,256))`,
 * `frame/256.0`, and leaves `cv2.flip(frame,1)` next to flip_pose commented out, :98-117).  The decisions flip, rotation,
 * scale and shift of a frame are those of pl_pose_augment_gather for the same (seed, epoch, row_id): frame, 2-D pose and 3-D
 * pose of a dataset row always agree.  jitter_sigma is pose noise and touches no frame.
 *   src [N][Hs][Ws][3] uint8 or fp32 -> out [n][Ho][Wo][3] fp32; sample k reads frame s = src_idx[k] (k when src_idx is NULL)
 *   with the draws of row_id[k].  Output pixel (i, j), every stage whose parameter is 0 skipped:
 *     u = (j + 0.5) / Wo, v = (i + 0.5) / Ho          (pixel centres, image-normalised: the 2-D pose's coordinates)
 *     u -= tx, v -= ty;  u = (u - cx) / sc + cx, v likewise;  (du, dv) = (u - cx, v - cy): u = (c du + s dv) + cx,
 *     v = (-s du + c dv) + cy;  flipped: u = 1 - u    (the pose transform undone in reverse order)
 *     xs = u Ws - 0.5, ys = v Hs - 0.5;  outside [-0.5, Ws - 0.5] x [-0.5, Hs - 0.5]: `fill` on all three channels
 *     else clamp to [0, Ws - 1] x [0, Hs - 1], x0 = floor(xs), x1 = min(x0 + 1, Ws - 1), y likewise, and
 *     value = scale * ((1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11))
 *   With aug NULL or all stages off this is bilinear resizing in cv2.resize's half-pixel convention (no antialiasing).
 *   Every operation is rounded on its own; the flip is taken as xs = (Ws - 1) - xs and, with shift, scale and rotation all
 *   off, xs = (j + 0.5) (Ws / Wo) - 0.5 (ys likewise), so a same-size resize copies scale * p exactly and a flip mirrors it.
 * A frame flip mirrors about the image centre: p_flip > 0 with flip_offset != 1 is PL_EINVAL; the other PLPoseAug checks are
 * pl_pose_augment_gather's.  C != 3 and non-positive sizes are PL_ESHAPE, a null table PL_EINVAL; an s outside [0, N) gives a
 * NaN frame on the device and PL_EINVAL on the host.  row_id may be NULL when aug is. */
enum { PL_FRAME_U8 = 0, PL_FRAME_F32 = 1 };
typedef struct PLFrameWarp {
  const void* src;          /* [N][Hs][Ws][C] */
  int32_t src_dtype;        /* PL_FRAME_U8 or PL_FRAME_F32 */
  int32_t C;                /* 3 */
  int64_t N, Hs, Ws;
  const int64_t* src_idx;   /* [n] or NULL */
  const int64_t* row_id;    /* [n] */
  int64_t n;
  float* out;               /* [n][Ho][Wo][C] */
  int64_t Ho, Wo;
  float scale;              /* the reference's frame/256.0: 1/256 for uint8 tables; 1 keeps fp32 values */
  float fill;               /* value of pixels whose source position lies outside the frame */
  const PLPoseAug* aug;     /* NULL: plain resize */
  uint64_t epoch;
} PLFrameWarp;
/* pl_frame_warp_gather: one launch on `stream`; no allocation, no synchronisation.
 * pl_frame_warp_host: the same inline text compiled for the CPU, on host pointers (a test hook). */
int pl_frame_warp_gather(const PLFrameWarp* a, void* stream);
int pl_frame_warp_host(const PLFrameWarp* a);

/* ---- person-centred crop taken from each row's 2-D pose (csrc/frame_crop.h has the definition) --------------------------
 * The reference crops "using the gt 2d as bounding box" (phase3_direct/my_HybrIK/H36_dataset.py:120-126) with a slice
 * min(0, ..) : max(1000, ..) that always selects the whole frame; without a crop the entry points above reproduce that.
 * Here the box is real and rides in the same two launches.  Box of a row, from its SOURCE 2-D pose a[17][2]
 * (image-normalised, x right and y down) and the source frame size (Hs, Ws):
 *   ex = (xmax - xmin) Ws, ey = (ymax - ymin) Hs over the 17 joints;  side = max(ceil(margin max(ex, ey)), min_side)
 *   centre PL_CROP_BBOX: ccx = (0.5 (xmin + xmax)) Ws, ccy = (0.5 (ymin + ymax)) Hs;  PL_CROP_ROOT: ccx = a[0][0] Ws, ccy = a[0][1] Hs
 *   x0 = rint(ccx - 0.5 side), y0 = rint(ccy - 0.5 side)      integers (ties to even), may be negative or past the frame
 * A non-finite coordinate anywhere in the pose, or a side above 2^20, makes the box NaN.  boxes [n][4] fp32 = (x0, y0, side, side).
 * Pose: a'x = (ax Ws - x0) / side, a'y = (ay Hs - y0) / side, in front of every augmentation stage, which then run unchanged
 * on a' ((cx, cy) = (0.5, 0.5) is the crop's centre; p_flip > 0 needs flip_offset 1); the 3-D pose is untouched.  A transform
 * (the _t forms) still applies last: its statistics must then be statistics of crop coordinates.
 * Frame: (u, v) of pl_frame_warp_gather are crop-normalised and the source position goes through the crop-local one,
 *   xl = u side - 0.5 (shift, scale and rotation all off: xl = (j + 0.5) (side / Wo) - 0.5);  flipped: xl = (side - 1) - xl;
 *   xs = xl + x0   (ys likewise), then the border rule and the taps of the FRAME: what lies outside it is `fill`.
 * Exact in fp32: side == Wo == Ho copies scale * frame[y0:y0+Ho, x0:x0+Wo], with a flip its mirror image, and
 * side == 2 Wo == 2 Ho is the 2 x 2 block mean.  A NaN box gives a NaN frame and a NaN 2-D pose.  The frame launch computes
 * the box from x2d by the same inline text as the pose launch: the two agree bit for bit without talking to each other.
 * margin not finite or <= 0, min_side < 1, not an integer or above 2^20, and a centre out of range are PL_EINVAL; Hs, Ws
 * outside [1, 2^22] (or, for a frame warp, other than the table's) PL_ESHAPE. */
enum { PL_CROP_BBOX = 0, PL_CROP_ROOT = 1 };
typedef struct PLPoseCrop {
  float margin;      /* box side = margin x the larger extent of the pose, in source pixels; > 0 */
  int32_t centre;    /* PL_CROP_BBOX: the middle of the pose's extent; PL_CROP_ROOT: joint 0 (the reference's choice, :126) */
  float min_side;    /* smallest side, source pixels: an integer in [1, 2^20] */
  int32_t reserved;  /* 0 */
  int64_t Hs, Ws;    /* the source frame the image-normalised poses refer to */
} PLPoseCrop;
/* The crop forms of the pose gathers: the same arguments, then crop and boxes [n][4] (an output).  crop NULL: the call IS the
 * entry point without _crop (same kernel instantiation, boxes not read).  A bad source index gives a NaN box. */
int pl_pose_augment_gather_crop(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                                const PLPoseCrop* crop, float* boxes, void* stream);
int pl_pose_augment_gather_crop_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                  int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                                  const float* sub_a, const float* div_a, const float* sub_b, const float* div_b,
                                  const PLPoseCrop* crop, float* boxes, void* stream);
int pl_pose_augment_host_crop(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                              int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                              const PLPoseCrop* crop, float* boxes);
int pl_pose_augment_host_crop_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                                const float* sub_a, const float* div_a, const float* sub_b, const float* div_b,
                                const PLPoseCrop* crop, float* boxes);
/* The crop form of the frame warp.  x2d: the rows' SOURCE 2-D poses, indexed like the frames: [N][34] read through src_idx,
 * or a gathered [n][34] block when src_idx is NULL.  crop NULL: the call IS pl_frame_warp_gather (x2d not read). */
int pl_frame_warp_gather_crop(const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d, void* stream);
int pl_frame_warp_host_crop(const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d);
/* boxes [n][4] of poses x2d [n][34] alone: one launch; _host: the same inline text on host pointers. */
int pl_pose_crop_boxes(const float* x2d, int64_t n, const PLPoseCrop* crop, float* boxes, void* stream);
int pl_pose_crop_boxes_host(const float* x2d, int64_t n, const PLPoseCrop* crop, float* boxes);
/* Poses p [n][17][2] between image and crop coordinates by boxes [n][4]: invert = 0: out = (p W - x0) / side (W = Ws for x,
 * Hs for y); invert != 0: out = (p side + x0) / W.  offset = 0 leaves x0, y0 out: both maps are affine per element, so the
 * backward pass of either is the same call with offset = 0 on the incoming gradient (its factor, W / side or side / W, alone).
 * out may overlap neither input.  One launch. */
int pl_crop_poses(const float* p, const float* boxes, int64_t n, int64_t Hs, int64_t Ws, int invert, int offset, float* out,
                  void* stream);
int pl_crop_poses_host(const float* p, const float* boxes, int64_t n, int64_t Hs, int64_t Ws, int invert, int offset, float* out);

/* ---- loss / metric / optimiser -------------------------------------------------- */
/* torch.nn.MSELoss(reduction="mean") + its backward  train_1.py:37,94-95.
 * n elements; dpred = grad_scale * 2 (pred - tgt) / n; loss_out: 1 device float.
 * scratch: >= pl_mse_scratch_bytes(n). dpred may be NULL (validation). */
size_t pl_mse_scratch_bytes(int64_t n);
int pl_mse_fwd_bwd(const float* pred, const float* tgt, int64_t n, float grad_scale,
                   float* dpred, float* loss_out, void* scratch, void* stream);

/* torch.nn.L1Loss(reduction="mean") terms of TriangleLoss (phase5_loop/losses.py:10-62; the LinearModel-era
 * copy phase5_loop/train_5 copy.py:34-86), ALL terms of one call in one launch pair:
 * losses[t] = mean |a_t - b_t| over n_t elements; gradients, where wanted, da_t = grad_scale *
 * sign(a_t - b_t) / n_t and db_t = -da_t (sign(0) = 0, as torch).  terms: HOST array of nterms <=
 * PL_L1_MAX_TERMS descriptors holding device pointers; losses: nterms device floats;
 * scratch >= pl_l1_scratch_bytes(nterms). */
#define PL_L1_MAX_TERMS 8
typedef struct PLL1Term {
  const float* a;
  const float* b;
  int64_t n;
  float* da; /* or NULL */
  float* db; /* or NULL */
} PLL1Term;
size_t pl_l1_scratch_bytes(int nterms);
int pl_l1_terms_fwd_bwd(const PLL1Term* terms, int nterms, float grad_scale, float* losses,
                        void* scratch, void* stream);

/* loss_MPJPE  train_1.py:19-23,100: metric[j] += sum_b ||pred[b][j] - tgt[b][j]||_2.
 * pred/tgt [B][joints][3]; metric [joints] device fp32, accumulated in place. */
size_t pl_mpjpe_scratch_bytes(int64_t B, int64_t joints);
int pl_mpjpe_accum(const float* pred, const float* tgt, int64_t B, int64_t joints,
                   float* metric, void* scratch, void* stream);
/* The same on tensors in a model's space: with (sub, div) [3 joints] given (joints <= 32), prediction and target are taken
 * back as they are loaded, x = y div[c] + sub[c] (pl_pose_affine's inverse, its div == 0 rule included), so the metric is
 * in the raw units.  Both NULL: pl_mpjpe_accum, the same kernel instantiation. */
int pl_mpjpe_accum_t(const float* pred, const float* tgt, int64_t B, int64_t joints, const float* sub_or_null,
                     const float* div_or_null, float* metric, void* scratch, void* stream);

/* ---- evaluation: MPJPE, N-MPJPE, P-MPJPE per pose and joint; sums and PCK counts per group --------------------------
 * The reference reports protocol-1 MPJPE only (train_1.py:19-23,100-104); these are the other columns of the usual
 * Human3.6M table.  pred / tgt [B][J][3] fp32, 3 <= J <= 32, 16-byte aligned.  Per pose, with rows P_j, T_j:
 *   err[0][b][j] = ||P_j - T_j||                                             MPJPE
 *   err[1][b][j] = ||s P_j - T_j||,  s = sum P.T / sum P.P (0 if sum P.P = 0; no centring)            N-MPJPE
 *   err[2][b][j] = ||a R (P_j - muP) + muT - T_j||                           P-MPJPE
 * where R is the best PROPER rotation of the centred prediction P0 onto the centred target T0 (a reflected prediction is
 * not flipped back: the SVD recipe with the determinant fix) and a = tr(R P0^T T0) / ||P0||^2 the best scale (0 if
 * ||P0||^2 = 0: a collapsed prediction is scored against the target's centroid, a collapsed target scores 0).  A NaN in a
 * pose makes that pose's N-MPJPE, P-MPJPE and aligned outputs NaN (MPJPE: at the joints that hold one) and touches no
 * other pose.  aligned_or_null [B][J][3]: a R (P_j - muP) + muT.
 * One launch, one lane per pose, no atomics: the same inputs give the same bits.
 * pl_pose_errors_host: the same inline arithmetic compiled for the CPU, on host pointers (a test hook). */
int pl_pose_errors(const float* pred, const float* tgt, int64_t B, int64_t J, float* err /* [3][B][J] */,
                   float* aligned_or_null, void* stream);
int pl_pose_errors_host(const float* pred, const float* tgt, int64_t B, int64_t J, float* err, float* aligned_or_null);
/* pl_pose_errors on tensors in a model's space: with (sub, div) [3 J] given, prediction and target are taken back as they
 * are loaded, x = y div[c] + sub[c] (pl_pose_affine's inverse), so errors, alignment and the aligned pose are those of the
 * raw poses.  Both NULL: pl_pose_errors, the same kernel instantiation. */
int pl_pose_errors_t(const float* pred, const float* tgt, int64_t B, int64_t J, const float* sub_or_null,
                     const float* div_or_null, float* err /* [3][B][J] */, float* aligned_or_null, void* stream);
/* Accumulate err [3][B][J] (pl_pose_errors) into per-group totals, in place:
 *   sums   [G][3][J]     fp32   += sum of errors of the poses of group g
 *   counts [G][3][T][J]  int64  += number of those errors <= thr[t] (inclusive)        (may be NULL when n_thr = 0)
 *   n_poses [G + 1]      int64  += poses of group g; cell G counts the poses whose id is outside [0, G), which add to
 *                                  nothing else (the host reports them; nothing traps on the device)
 * group_or_null [B] int32 (NULL: every pose is group 0); 1 <= groups <= 32; thr_or_null [n_thr] fp32, 0 <= n_thr <= 32.
 * Two launches (per-chunk partials into scratch >= pl_pose_metrics_scratch_bytes(B, J, groups, n_thr), then one thread
 * per cell), no atomics, a fixed order of every sum. */
size_t pl_pose_metrics_scratch_bytes(int64_t B, int64_t J, int groups, int n_thr);
int pl_pose_metrics_accum(const float* err, int64_t B, int64_t J, const int32_t* group_or_null, int groups,
                          const float* thr_or_null, int n_thr, float* sums, int64_t* counts, int64_t* n_poses,
                          void* scratch, void* stream);

/* ---- evaluation with missing joints: per-pose joint weights (visibility) ----------------------------------------------
 * weights [B][J] fp32, 4-byte aligned.  For pose b let w = weights[b], V = { j : w_j > 0 } and W = sum_V w_j.  A weight that
 * is not > 0 (zero, negative or NaN) means "not visible"; nothing validates weights on the host, so nothing synchronises.
 * err stays [3][B][J] and is written for every joint, visible or not:
 *   err[0] MPJPE     ||P_j - T_j||, unchanged
 *   err[1] N-MPJPE   ||s P_j - T_j||,  s = sum_V w_j P_j.T_j / sum_V w_j P_j.P_j   (0 when the denominator == 0)
 *   err[2] P-MPJPE   ||a R (P_j - muP) + muT - T_j||,  muP = sum_V w_j P_j / W and muT likewise,
 *                    M = sum_V w_j (P_j - muP)(T_j - muT)^T,  R = Horn's best proper rotation of N(M) (the same Jacobi
 *                    route),  a = lambda / sum_V w_j ||P_j - muP||^2   (0 when that sum == 0)
 * aligned = a R (P_j - muP) + muT for every joint: an invisible joint is carried by the transform fitted on the visible
 * ones, and its error says how far the occluded joint lands.
 * Sums over V are SELECTS, not products: a joint outside V is not read into any whole-pose sum, so a NaN or infinity at an
 * invisible joint of the prediction or the target reaches only that joint's own three error cells and its aligned
 * coordinates.  (The criterion's row weights multiply, there a zero weight times a NaN is a NaN; a NaN-coded missing ground
 * truth is exactly the case this is for.)  A NaN at a visible joint behaves as in pl_pose_errors.  Everything centred is
 * formed from differences to the FIRST VISIBLE joint: a collapsed visible subset is exactly 0 and an offset of 1000 m
 * costs nothing.
 * Degenerate: W == 0 (no visible joint): s = 0, a = 0, both centroids 0, finite outputs for finite inputs.  One visible
 * joint: a = 0, that joint's P-MPJPE is 0.  Two visible joints, or visible joints on a line: the rotation about the line
 * is undetermined; results are finite, the split of the error over the invisible joints is not pinned.
 * c w (c > 0) gives the results of w, and all-ones weights those of pl_pose_errors, to rounding.
 * weights_or_null == NULL and (sub, div) [3 J] both NULL: pl_pose_errors / pl_pose_errors_t, the same kernel
 * instantiations, bit for bit.  pl_pose_errors_w_host: the same inline arithmetic on host pointers (a test hook). */
int pl_pose_errors_w(const float* pred, const float* tgt, int64_t B, int64_t J, const float* weights_or_null,
                     const float* sub_or_null, const float* div_or_null, float* err /* [3][B][J] */, float* aligned_or_null,
                     void* stream);
int pl_pose_errors_w_host(const float* pred, const float* tgt, int64_t B, int64_t J, const float* weights_or_null,
                          const float* sub_or_null, const float* div_or_null, float* err, float* aligned_or_null);
/* pl_pose_metrics_accum as a masked mean.  With v_bj = (weights[b][j] > 0), per group g of the poses:
 *   sums   [G][3][J]     += sum_b v_bj err[m][b][j]
 *   counts [G][3][T][J]  += number of b with v_bj and err[m][b][j] <= thr[t]
 *   n_valid [G][J] int64 += sum_b v_bj                               (8-byte aligned)
 *   n_poses [G + 1]      += poses of group g, fully invisible ones included (cell G: ids outside [0, G))
 * The weights' magnitudes matter to the alignment only; the weight is read beside the error it gates and selects, so a
 * non-finite error behind a weight that is not > 0 is in nothing.  The same two launches (the visible counts are one more
 * job of the first grid), no atomics, a fixed order of every sum; scratch >= the _w_ size below, which is
 * pl_pose_metrics_scratch_bytes plus 4 G J bytes per chunk. */
size_t pl_pose_metrics_w_scratch_bytes(int64_t B, int64_t J, int groups, int n_thr);
int pl_pose_metrics_accum_w(const float* err, const float* weights, int64_t B, int64_t J, const int32_t* group_or_null,
                            int groups, const float* thr_or_null, int n_thr, float* sums, int64_t* counts, int64_t* n_poses,
                            int64_t* n_valid, void* scratch, void* stream);

/* *counter += delta on the stream (one thread).  The optimizer of a step replayed from a hipGraph keeps its step count on
 * the device: pl_adamw_flat_dev reads t = t_base + *t_dev, this call ticks it behind the update (arena.FlatAdam for the
 * conv models: torch.optim.Adam(model.parameters(), lr) of phase4_joined/train.py:39, train_5 copy.py:105-109). */
int pl_counter_add(uint64_t* counter, int64_t delta, void* stream);

/* flip_pose  phase3_direct/my_HybrIK/utils.py:372-396 (used by train_1.py:89-92,128-134 when Flip):
 * out = horizontal flip of in, both [B][17][D], D = 2 (x -> 1-x) or 3 (x -> -x), left/right joints
 * [4,5,6,11,12,13] <-> [1,2,3,14,15,16] swapped.  Out of place. */
int pl_flip_pose(const float* in, float* out, int64_t B, int64_t joints, int64_t D, void* stream);

/* The training-mode Flip branch of the phase5 cycle step, phase5_loop/train_5 copy.py:174-199:
 *   y = (flip_pose(a) + b) / 2      -> pl_flip_pose_ex(a, b, y, ..., x_offset = (D == 2 ? 1 : 0), scale = 0.5)
 *   its backward da = flip'(g) / 2  -> pl_flip_pose_ex(g, NULL, da, ..., x_offset = 0, scale = 0.5)
 * out[b][j][d] = ((d == 0 ? x_offset - in[b][src(j)][0] : in[b][src(j)][d]) + (addend ? addend[b][j][d] : 0)) * scale,
 * src = the left/right joint swap of pl_flip_pose.  addend may be NULL.  Out of place. */
int pl_flip_pose_ex(const float* in, const float* addend, float* out, int64_t B, int64_t joints, int64_t D,
                    float x_offset, float scale, void* stream);

/* torch.flip(frame, (3,)) of train_5 copy.py:176 (NCHW dim 3 = width) on NHWC frames: out[b][h][w][c] = in[b][h][W-1-w][c]. */
int pl_flip_w_nhwc(const float* in, float* out, int64_t B, int64_t H, int64_t W, int64_t C, void* stream);

/* Flip test-time augmentation, (flip_pose(model(flip_pose(x))) + model(x)) / 2 -- the intent of
 * train_1.py:128-134 and phase5_loop/train_5 copy.py:160-171 -- around ONE eval forward of 2B rows:
 *   pack : xx [2B][17][D]: rows [0,B) = x, rows [B,2B) = flip_pose(x)
 *   merge: y [B][17][D] = (yy[0:B) + flip_pose(yy[B:2B))) / 2 */
int pl_flip_tta_pack(const float* x, float* xx, int64_t B, int64_t joints, int64_t D, void* stream);
int pl_flip_tta_merge(const float* yy, float* y, int64_t B, int64_t joints, int64_t D, void* stream);

/* torch.optim.AdamW.step  train_1.py:39,96 over one flat arena (p, g, m, v of n floats).
 * t = 1-based step count; g is multiplied by grad_scale first (1/world_size after a
 * sum all-reduce). */
int pl_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t t, float grad_scale, void* stream);

/* The same step with its two per-step inputs read from device memory, so that a captured graph advances by itself:
 * t = t_base + *t_dev (t_dev: a step counter such as PLDesc.step_dev, incremented elsewhere in the graph) and
 * lr = *lr_dev (the host-side LR scheduler writes it).  Bias corrections are derived on the device from t by the
 * code pl_adamw_flat runs, so a replayed step equals the eager one bit for bit. */
int pl_adamw_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev,
                      float beta1, float beta2, float eps, float weight_decay, int64_t t_base,
                      const uint64_t* t_dev, float grad_scale, void* stream);

/* The step that ALSO refreshes the GEMM operand planes of the 1024-wide weight matrices (PL_F16X3: two fp16 planes,
 * PL_BF16: the bf16 shadow) while the updated parameters are in registers: the forward of the next step then needs
 * no weight split of its own (PLDesc.wplanes / wplanes_valid).  seg[q]: floats [offset, offset + numel) of the arena
 * (both multiples of 4) -> plane h (and l) of numel 16-bit elements each.  lr_dev / t_dev as in pl_adamw_flat_dev, or
 * both NULL (lr, t by value). */
#define PL_ADAMW_MAX_SEGS 8
typedef struct PLAdamWSeg {
  int64_t offset, numel;
  void* h;
  void* l;              /* kind 2 only */
} PLAdamWSeg;
typedef struct PLAdamWPlanes {
  int32_t nseg;
  int32_t kind;         /* 1 bf16, 2 fp16 pair */
  float scale;          /* the weight planes' power-of-two scale: pl_weight_plane_scale() */
  int32_t reserved;
  PLAdamWSeg seg[PL_ADAMW_MAX_SEGS];
} PLAdamWPlanes;
int pl_adamw_flat_planes(float* p, const float* g, float* m, float* v, int64_t n, float lr, const float* lr_dev,
                         float beta1, float beta2, float eps, float weight_decay, int64_t t, const uint64_t* t_dev,
                         float grad_scale, const PLAdamWPlanes* planes, void* stream);
/* ---- gradient-norm clipping and non-finite skip over a flat gradient arena --------------------
 * nn.utils.clip_grad_norm(model.parameters(), max_norm=1) between loss.backward() and optimizer.step()
 * (phase1_lifting/main.py:465-470, MaxNormConctraint), without a host decision: pl_grad_norm_clip writes a small device
 * record, the *_clip forms of the flat AdamW step read it.  The gradient arena itself is never rewritten.
 *   norm    = |grad_scale| * sqrt(sum of g^2 over the ranges), the sum in fp64 (a product of two fp32 values is exact
 *             there: no square overflows or underflows), rounded to fp32 once
 *   coef    = min(1, max_norm / (norm + 1e-6f)) in fp32, torch's formula (NaN stays NaN); 1 when clip == 0
 *   finite  = isfinite(norm)
 *   skip    = skip_nonfinite && !finite: the AdamW launches behind this record leave p, m, v bitwise untouched (and still
 *             write the operand planes, from the unchanged parameters)
 *   skipped = number of steps skipped so far (this call adds 1 when skip); AdamW's bias corrections use t - skipped,
 *             which is what a loop that does not call optimizer.step() on such a step gives
 * The caller zeroes the record once and keeps it for the life of the optimizer (it is baked into captured graphs). */
typedef struct PLClipRecord {
  float norm;
  float coef;
  uint32_t finite;
  uint32_t skip;
  uint64_t skipped;
} PLClipRecord;
/* [lo, hi) in floats of the arena; lo a multiple of 4, hi arbitrary; ascending and disjoint.  Nothing outside the ranges
 * is read: a NaN in an inactive slot (BN=False, a frozen parameter, no gradient) does not matter. */
typedef struct PLGradRange {
  int64_t lo, hi;
} PLGradRange;
#define PL_GRAD_NORM_MAX_RANGES 1024
size_t pl_grad_norm_scratch_bytes(int nranges);
/* g: the gradient arena of n floats, 16-byte aligned.  clip != 0: max_norm (>= 0) by value, or *max_norm_dev when that
 * pointer is set (captured graphs, as lr / lr_dev).  record and scratch (>= pl_grad_norm_scratch_bytes(nranges)) 8-byte
 * aligned.  Per-workgroup fp64 partials, then one workgroup sums them in a fixed order: no atomics, a repeated call gives
 * the same bits. */
int pl_grad_norm_clip(const float* g, int64_t n, const PLGradRange* ranges, int nranges, float grad_scale, int clip,
                      float max_norm, const float* max_norm_dev, int skip_nonfinite, PLClipRecord* record, void* scratch,
                      void* stream);
/* pl_adamw_flat / pl_adamw_flat_dev / pl_adamw_flat_planes with the record of the pl_grad_norm_clip launched before them on
 * the stream: the gradient is multiplied by grad_scale * clip->coef (one fp32 product), t is t - clip->skipped, and nothing
 * is updated when clip->skip.  clip == NULL: exactly the call without the suffix. */
int pl_adamw_flat_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int64_t t, float grad_scale, const PLClipRecord* clip, void* stream);
int pl_adamw_flat_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1,
                           float beta2, float eps, float weight_decay, int64_t t_base, const uint64_t* t_dev,
                           float grad_scale, const PLClipRecord* clip, void* stream);
int pl_adamw_flat_planes_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, const float* lr_dev,
                              float beta1, float beta2, float eps, float weight_decay, int64_t t, const uint64_t* t_dev,
                              float grad_scale, const PLAdamWPlanes* planes, const PLClipRecord* clip, void* stream);

/* pl_adamw_flat_planes_clip with the averaged weights of [p, p + n) kept in the same launch (ema->e: beside p).  ema == NULL:
 * exactly pl_adamw_flat_planes_clip -- the kernels it always launched, the bits it always wrote. */
int pl_adamw_flat_planes_clip_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, const float* lr_dev,
                                  float beta1, float beta2, float eps, float weight_decay, int64_t t, const uint64_t* t_dev,
                                  float grad_scale, const PLAdamWPlanes* planes, const PLClipRecord* clip, const PLEma* ema,
                                  void* stream);

/* Layout of the caller-owned weight-plane buffer PLDesc.wplanes: pl_wplanes_bytes() bytes (0: this descriptor has no
 * planes path); the planes of hidden layer l (1 <= l < n_hidden) start at byte (l - 1) * pl_wplanes_layer_bytes(d):
 * plane h, then (PL_F16X3) plane l, hidden*hidden 16-bit elements each, row-major like the weight. */
size_t pl_wplanes_bytes(const PLDesc* d);
size_t pl_wplanes_layer_bytes(const PLDesc* d);
float pl_weight_plane_scale(void);
int pl_wplanes_refresh(const PLDesc* d, void* stream);   /* planes <- current parameters (wplanes_valid is ignored) */

/* ---- PL_F16X3 range guard ---------------------------------------------------------- */
/* PL_F16X3 stores activations, weights and conv-path feature maps as fp16 planes at STATIC scales (activations 1, weights
 * 16, conv-path maps 1/64): a finite fp32 value v with |S v| > 65504 becomes inf in its plane and NaN in the next GEMM.
 * With a record set, every kernel that writes such a plane also notes that it saw one: record[site] (the caller's
 * PL_RANGE_SITES device words, zeroed by the caller) takes, by an atomic maximum, the fp32 bit pattern of the largest
 * UNSCALED |v| that left the range at that site; 0 = clean.  inf / NaN sources are not recorded, planes with a scale
 * chosen on the device (dz, dlogits) cannot leave the range, and the planes themselves are written exactly as without a
 * record.  pl_range_monitor sets the record of the CALLING THREAD's later calls (NULL, the initial state: none); the pointer
 * is read when a call enqueues its launches, so it is part of a captured graph and must outlive it.  Returns PL_OK. */
#define PL_RANGE_SITES 16
#define PL_RANGE_SITE_LIFTER_ACT 0     /* .. 7: output of the lifter's hidden layer l at min(l, 7) (scale 1)       */
#define PL_RANGE_SITE_LIFTER_WEIGHT 8  /* the lifter's 1024-wide weight planes (scale 16)                          */
#define PL_RANGE_SITE_CONV_ACT 9       /* conv-path feature maps (scale pl_conv_act_plane_scale())                 */
#define PL_RANGE_SITE_CONV_WEIGHT 10   /* pl_planes_split* at scale 16: the conv path's weights                     */
#define PL_RANGE_SITE_SPLIT 11         /* pl_planes_split*, pl_gemm_planes at any other scale                       */
int pl_range_monitor(void* record_or_null);

/* ---- building blocks exported for tests ------------------------------------------ */
/* C[M][N] = op(A) op(B) on the fp32 MFMA path.
 * layout 0 (NT): A [M][K], B [N][K]   (forward  z = a W^T)
 * layout 1 (NN): A [M][K], B [K][N]   (backward da = dz W)
 * layout 2 (TN): A [K][M], B [K][N]   (backward dW = dz^T a)
 * bias [N] or NULL is added to every row. split_k > 1 is allowed for layout 2 only and
 * needs slab scratch of split_k*M*N floats (NULL otherwise). */
int pl_gemm_f32(int layout, const float* A, const float* B, float* C, int64_t M,
                int64_t N, int64_t K, const float* bias, int split_k, float* slabs,
                void* stream);
/* the same with the arithmetic chosen (PLDtype); bf16 modes apply to whole 128x128x32 tiles only */
int pl_gemm_arith(int layout, int arith, const float* A, const float* B, float* C, int64_t M,
                  int64_t N, int64_t K, const float* bias, int split_k, float* slabs,
                  void* stream);

/* The same product computed the way the PL_F16X3 / PL_BF16-storage lifter computes its 1024-wide Linears: A and B are
 * split into 16-bit operand planes in `scratch` (the lifter's own producers -- BatchNorm apply / backward, the weight
 * split -- write planes directly), then one planes GEMM (LDS-DMA staging, no split work in the loop).  mode PL_F16X3:
 * scale_a, scale_b are the power-of-two tensor scales (|scale * x| must stay below 65504); mode PL_BF16: one bf16 plane
 * per operand, scales ignored.  M, N % 128 == 0, K % 32 == 0. */
size_t pl_gemm_planes_scratch_bytes(int64_t M, int64_t N, int64_t K);
int pl_gemm_planes(int layout, int mode, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                   const float* bias, float scale_a, float scale_b, void* scratch, void* stream);
/* The planes GEMM on operands that already ARE planes (1x1 convolutions of the conv path: forward NT on
 * [pixels][Cin] x [Cout][Cin], data gradient NT on dz [pixels][Cout] x W^T [Cin][Cout], weight gradient TN over the
 * pixels; reference phase4_joined/Resnet.py:56-63 and their autograd).  Layout as pl_gemm_f32 (0 NT, 1 NN, 2 TN);
 * a_plane / b_plane: elements between the two fp16 planes of an operand (unused for PL_BF16); lda / ldb: row strides
 * of the plane matrices in elements (% 8 == 0).  C = out_scale * [dyn_inv[0] *] (A B) (+ bias): out_scale = 1 / (S_A S_B),
 * dyn_inv a device scalar or NULL.  Any M; N % 8 == 0 (TN: M % 8 == 0 too); K % (32 * splits) == 0.  splits =
 * pl_gemm_planes_splits(M, N, K) > 1 needs slabs of splits * M * N floats (K slices summed in order into C).
 * stat (optional, unsplit problems; also on pl_conv2d_planes_fwd): [2][pl_gemm_stat_groups(M)][N] -- the epilogue also emits
 * training-mode BatchNorm partial statistics of C, for pl_bn_train_fwd_ex. */
int pl_gemm_planes_splits(int64_t M, int64_t N, int64_t K);
int pl_gemm_stat_groups(int64_t M);   /* 64-row statistics groups a GEMM epilogue emits for M rows (2 per 128-row tile) */
/* KxK convolutions the same way (implicit GEMM: the loader waves gather the NHWC input planes tap by tap, padding pixels
 * read as zeros; reference Resnet.py:58-60 conv2 and its autograd).  x_planes: planes of x [B][H][W][Cin], Cin % 32 == 0;
 * w_planes: planes of the OHWI kernel [Cout][KH*KW*Cin]; y [B][Ho][Wo][Cout] fp32.  The data gradient of a stride-1
 * convolution is the same call on the planes of dz with the kernel flipped and transposed ([Cin][KH][KW][Cout], pad
 * KH-1-pad).  wgrad: dw [Cout][KH*KW*Cin] = sum over output pixels of dz (planes [B][Ho][Wo][Cout]) x gathered x; slabs:
 * pl_gemm_planes_splits(Cout, KH*KW*Cin, B*Ho*Wo) * Cout * KH*KW*Cin floats when that is > 1.  out_scale / dyn_inv as above. */
int pl_conv2d_planes_fwd(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                         const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride, int pad,
                         float* y, float out_scale, const float* dyn_inv, float* stat, void* stream);
/* The head's last link on planes: the 3-D soft-argmax backward writing dlogits (4.5 GB at B = 256) as operand planes for the
 * final 1x1 convolution's gradient GEMMs (dlogits may be NULL), and the bias gradient as column sums of those planes.
 * PL_F16X3: dl_scale = {S, 1/S} on the device, S a power of two the caller derives from |dlogit| <= 2 max sum_c |g_c|. */
int pl_softargmax3d_nhwc_bwd_ex(const float* logits, const float* stats, const float* gcoords, int64_t B, int64_t J,
                                int64_t H, int64_t W, float* dlogits, void* dl_planes, int planes_mode,
                                const float* dl_scale, void* stream);
int pl_colsum_planes(const void* planes, int planes_mode, int64_t rows, int64_t cols, const float* inv_scale, float* out,
                     void* scratch, void* stream);
/* nn.ConvTranspose2d(4, 2, 1, bias=False) forward the same way (Model.py:47-63): four 2x2-tap gathers at the input
 * resolution, one per output parity, stored straight into y [B][2H][2W][Cout]; wsub_planes = planes of
 * conv.deconv_subkernels(weight) [4][Cout][2][2][Cin].  Its data gradient is pl_conv2d_planes_fwd (4x4, stride 2, pad 1)
 * on the planes of dy, its weight gradient pl_conv2d_planes_wgrad with the roles of x and dy exchanged. */
int pl_deconv4x4s2_planes_fwd(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                              const void* wsub_planes, int64_t wsub_plane, int64_t Cout, float* y, float out_scale,
                              const float* dyn_inv, void* stream);
/* Eval-mode forms of the two: the Bottleneck's / the head's folded epilogue (BatchNorm on running statistics as
 * scale / shift, bias, ReLU, residual: pl_conv2d_nhwc_fwd's) applied to the convolution's result, which is written as fp32 (y,
 * may be NULL) and / or as operand planes for the next convolution (ep->y_planes, scale pl_conv_act_plane_scale(); NULL = none).
 * relu: 0 none, 1 ReLU then + resid, 2 + resid then ReLU.  Reference: Resnet.py:65-93, Model.py:47-69 under model.eval(). */
typedef struct PLPlanesEpilogue {
  const float* bias;      /* [Cout] or NULL */
  const float* scale;     /* [Cout] or NULL (with shift) */
  const float* shift;
  const float* resid;     /* [pixels][Cout] fp32 or NULL */
  int32_t relu;
  int32_t reserved;
  void* y_planes;         /* planes of the result (mode as the call's), or NULL */
} PLPlanesEpilogue;
int pl_conv2d_planes_fwd_ep(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                            const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride, int pad,
                            float* y, float out_scale, const PLPlanesEpilogue* ep, void* stream);
int pl_deconv4x4s2_planes_fwd_ep(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                 int64_t Cin, const void* wsub_planes, int64_t wsub_plane, int64_t Cout, float* y,
                                 float out_scale, const PLPlanesEpilogue* ep, void* stream);
int pl_conv2d_planes_wgrad(int mode, const void* dz_planes, int64_t dz_plane, const void* x_planes, int64_t x_plane,
                           int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH, int KW, int stride,
                           int pad, float* dw, float out_scale, const float* dyn_inv, float* slabs, void* stream);
/* The same two with separate strides and paddings along h and w, and -- forward -- an 8-channel input when KW % 4 == 0 (a 32-k
 * tile is then four neighbouring taps of one kernel row).  What this is for: the 7x7 / stride 2 / pad 3 stem on 3 input
 * channels (phase4_joined/Resnet.py:112-113,137) as a planes GEMM -- the frame padded to 4 channels and viewed as pixel PAIRS
 * [B][H][W/2][8], the kernel as 7 x 4 taps of 8 (zero where the pair window overhangs the 7 real taps), stride (2, 1),
 * padding 3 above and below, 2 pairs left and 1 right (pad_w / pad_w_right: W/2 outputs per row): conv.stem_planes. */
int pl_conv2d_planes_fwd_hw(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                            const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride_h, int stride_w,
                            int pad_h, int pad_w, int pad_w_right, float* y, float out_scale, const float* dyn_inv, float* stat,
                            void* stream);
int pl_conv2d_planes_fwd_ep_hw(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                               const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride_h, int stride_w,
                               int pad_h, int pad_w, int pad_w_right, float* y, float out_scale, const PLPlanesEpilogue* ep,
                               void* stream);      /* pl_conv2d_planes_fwd_ep with that geometry: the stem in eval mode */
int pl_conv2d_planes_wgrad_hw(int mode, const void* dz_planes, int64_t dz_plane, const void* x_planes, int64_t x_plane,
                              int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH, int KW, int stride_h,
                              int stride_w, int pad_h, int pad_w, int pad_w_right, float* dw, float out_scale,
                              const float* dyn_inv, float* slabs, void* stream);
int pl_gemm_planes_raw(int layout, int mode, const void* A, int64_t a_plane, int64_t lda, const void* B, int64_t b_plane,
                       int64_t ldb, float* C, int64_t M, int64_t N, int64_t K, const float* bias, float out_scale,
                       const float* dyn_inv, float* slabs, float* stat, void* stream);

/* ---- next row N1: fused softmax + integral soft-argmax ----------------------------------- */
/* Tail of Model_3D.forward  phase4_joined/Model.py:94-133 (ncoord 3, centred 1: (E/dim - 0.5)*2)
 * and of Model_2D.forward  phase5_loop/Model_2d.py:96-134 (ncoord 2, D 1, centred 0: E/dim).
 * logits [BJ][D][H][W] (BJ = batch*joints, W % 4 == 0): softmax over the D*H*W voxels of each
 * (batch, joint), then the expectation of the w / h / d index.  coords [BJ][ncoord] in (x, y, z)
 * order; stats [BJ][5] = {max, sum exp, Ex, Ey, Ez} is what the backward needs.
 * Backward: dlogits [BJ][D][H][W] from gcoords [BJ][ncoord]; re-reads logits, materialises nothing. */
/* {S, 1/S} (device, two floats) for pl_softargmax3d_nhwc_bwd_ex's fp16 planes of dlogits: S = the power of two that maps
 * the bound 2 max_rows sum_c |gcoords[row][c]| >= max |dlogit| into (2^13, 2^14]; a zero / non-finite bound gives 1. */
int pl_softargmax_dl_scale(const float* gcoords, int64_t rows, int ncoord, float* scale2, void* stream);
int pl_softargmax_fwd(const float* logits, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord,
                      int centred, float* coords, float* stats, void* stream);
int pl_softargmax_bwd(const float* logits, const float* stats, const float* gcoords, int64_t BJ,
                      int64_t D, int64_t H, int64_t W, int ncoord, int centred, float* dlogits,
                      void* stream);

/* ---- heat-map supervision in the soft-argmax heads (csrc/heatmap_target.h) ------------------------------------------
 * The reference's other loss, MSELoss(heatmap_hat, hm) (phase5_loop/train_5.py:130-142,188) against the dataset's Gaussian
 * target (phase3_direct/my_HybrIK/H36_dataset.py:148-202), with neither the normalised heat-map nor the target stored:
 *   target[BJ][ncoord]  the joints' target coordinates in the head's (x, y[, z]) <-> (W, H[, D]) order
 *   law[6]              HOST floats {alpha x, y, z, gamma x, y, z}: centre index mu_a = alpha_a * (t_a + gamma_a)
 *   sigma               window half = (ceil(6 sigma) made odd) / 2 <= 8, else PL_ESHAPE
 *   g                   exp(-sum_a (idx_a - mu_a)^2 / (2 sigma^2)) where |idx_a - rint(mu_a)| <= half on every axis, else 0
 * A non-finite centre makes that (b, j)'s sq, its stats[5..7] and its dlogits NaN and touches no other pair.
 * pl_heatmap_gaussian(_host): the dense target out[BJ][D][H][W] on the device / on the host (test hook, same arithmetic). */
int pl_heatmap_gaussian(const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, float sigma,
                        const float* law, float* out, void* stream);
int pl_heatmap_gaussian_host(const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, float sigma,
                             const float* law, float* out);
/* pl_softargmax_fwd / pl_softargmax3d_nhwc_fwd + sq[BJ] = sum_v (p_v - g_v)^2 in the same single read of the logits; coords
 * are bitwise the plain entry point's.  stats [BJ][8] = {max, sum exp, Ex, Ey, Ez, sum p^2, sum_win p g, sum_win g^2}. */
int pl_softargmax_hm_fwd(const float* logits, const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord,
                         int centred, float sigma, const float* law, float* coords, float* sq, float* stats, void* stream);
int pl_softargmax3d_nhwc_hm_fwd(const float* logits, const float* target, int64_t B, int64_t J, int64_t H, int64_t W,
                                float sigma, const float* law, float* coords, float* sq, float* stats, void* stream);
/* The backward passes with the heat-map term: gsq[BJ] is the upstream gradient of sq (masks and per-joint weights are the
 * caller's multiplication), dlogit_v += 2 gsq p_v (p_v - g_v - (sum p^2 - sum_win p g)).  gsq == 0 gives the plain
 * backward's values.  The _ex form writes fp32, planes or both like pl_softargmax3d_nhwc_bwd_ex; its fp16 dl_scale comes
 * from pl_softargmax_hm_dl_scale: the bound 2 max_rows (sum_c |gcoords| + 2 |gsq|). */
int pl_softargmax_hm_bwd(const float* logits, const float* target, const float* stats, const float* gcoords, const float* gsq,
                         int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, int centred, float sigma, const float* law,
                         float* dlogits, void* stream);
int pl_softargmax3d_nhwc_hm_bwd_ex(const float* logits, const float* target, const float* stats, const float* gcoords,
                                   const float* gsq, int64_t B, int64_t J, int64_t H, int64_t W, float sigma, const float* law,
                                   float* dlogits, void* dl_planes, int planes_mode, const float* dl_scale, void* stream);
int pl_softargmax_hm_dl_scale(const float* gcoords, const float* gsq, int64_t rows, int ncoord, float* scale2, void* stream);

/* ---- MyViT, the transformer lifter (phase1_lifting/baselineModel.py:220-362) ------------ */
/* The non-GEMM parts of its forward and backward (vit.hip); its Linears run on pl_gemm_f32 / pl_gemm_planes_raw.
 * T = B * seq token rows of H features, row-major.  Parameter gradients are reduced in a fixed order (per-256-row
 * partial sums in `scratch`, then one ordered pass): bitwise repeatable.
 *   pl_vit_embed_fwd : x = x2d W^T + b + pos[t % seq]   (x2d [T][in_d], W [H][in_d], pos [seq][H]); in_d <= 8
 *   pl_vit_embed_bwd : dWb [H*in_d + H] = dW (the parameter's layout), then db; dpos [seq][H] (NULL: not wanted);
 *                      dx2d [T][in_d] (NULL: not wanted; needs W)
 *   pl_vit_ln_fwd    : x_out = x + add (add may be NULL: no residual add, x_out unused), then nnorm chained
 *                      LayerNorms (0, 1 or 2: norm1 then mhsa.norm) -> y; stats [nnorm][2][T] = row mean about the row's
 *                      first element (exact for a large mean and a small spread), 1/std.
 *                      H % 4 == 0, H <= 1024, 16-byte aligned rows
 *   pl_vit_ln_bwd    : dx = dres (may be NULL) + the chained LayerNorm backward of dy; x is the first LayerNorm's
 *                      input; dgb [nnorm][2][H] = dgamma, dbeta of each LayerNorm; b1 is needed when nnorm == 2
 *   pl_vit_attn_fwd  : qkv [B*seq][3*heads*64] (q | k | v, "b n (h d)") -> o [B*seq][heads*64] =
 *                      softmax(scale q k^T) v per (sample, head); lse [B][heads][seq] for the backward.  seq <= 32,
 *                      dim_head == 64 (pl_vit_attn_supported)
 *   pl_vit_attn_bwd  : dqkv from qkv, lse and dO (P recomputed)
 *   pl_vit_gelu_*    : exact GELU 0.5 u (1 + erf(u / sqrt 2)); du = dy GELU'(u)
 *   pl_vit_head_fwd  : y = relu(z) W^T + b  (z [T][K], W [out_d][K]); K <= 256, out_d <= 4
 *   pl_vit_head_bwd  : dz = [!(z <= 0)] dy W (a NaN z passes, as torch); dWb [out_d*K + out_d] = dW, then db
 *   pl_vit_planes_dyn: PL_F16X3 operand planes of x [rows][cols] (cols % 4 == 0) in a [rows_pad][cols] carrier (rows
 *                      past `rows` zero: a padded contraction for the TN weight gradients) with S the power of two
 *                      that maps max |x| into [2^13, 2^14), chosen on the device; scale (device, 3 floats) = {S, 1/S,
 *                      other_scale[1] / S} (other_scale may be NULL: then 1/S).  scratch: pl_vit_planes_scratch_bytes() */
int pl_vit_attn_supported(int seq, int heads, int dim_head);
int pl_vit_embed_fwd(const float* x2d, int64_t T, int in_d, int seq, const float* W, const float* b, const float* pos,
                     int H, float* x, void* stream);
size_t pl_vit_embed_bwd_scratch_bytes(int64_t T, int in_d, int H);
int pl_vit_embed_bwd(const float* dx, const float* x2d, int64_t T, int in_d, int seq, int H, const float* W, float* dWb,
                     float* dpos, float* dx2d, void* scratch, void* stream);
int pl_vit_ln_fwd(const float* x, const float* add, int64_t T, int H, int nnorm, const float* g1, const float* b1,
                  const float* g2, const float* b2, float eps, float* x_out, float* y, float* stats, void* stream);
size_t pl_vit_ln_bwd_scratch_bytes(int64_t T, int H, int nnorm);
int pl_vit_ln_bwd(const float* dy, const float* dres, const float* x, const float* stats, int64_t T, int H, int nnorm,
                  const float* g1, const float* b1, const float* g2, float* dx, float* dgb, void* scratch, void* stream);
int pl_vit_attn_fwd(const float* qkv, int64_t B, int seq, int heads, int dim_head, float scale, float* o, float* lse,
                    void* stream);
int pl_vit_attn_bwd(const float* qkv, const float* lse, const float* dout, int64_t B, int seq, int heads, int dim_head,
                    float scale, float* dqkv, void* stream);
int pl_vit_gelu_fwd(const float* u, int64_t n, float* y, void* stream);
int pl_vit_gelu_bwd(const float* u, const float* dy, int64_t n, float* du, void* stream);
int pl_vit_head_fwd(const float* z, int64_t T, int K, const float* W, const float* b, int out_d, float* y, void* stream);
size_t pl_vit_head_bwd_scratch_bytes(int64_t T, int K, int out_d);
int pl_vit_head_bwd(const float* dy, const float* z, int64_t T, int K, const float* W, int out_d, float* dz, float* dWb,
                    void* scratch, void* stream);
size_t pl_vit_planes_scratch_bytes(void);
int pl_vit_planes_dyn(const float* x, int64_t rows, int64_t cols, int64_t rows_pad, const float* other_scale, float* scale,
                      void* planes, void* scratch, void* stream);
/* MyViT "bf16p" mode: the producers of the block Linears' operands also write a bf16 CARRIER of their output -- row-major
 * [rows_pad][cols] bf16 (cols: H, heads*64, 3*heads*64 or 4*H), rows_pad >= T, rows_pad % 32 == 0, the rows past T zero (the
 * padded contraction of the TN weight gradients), 16-byte aligned: a PL_BF16 operand of pl_gemm_planes_raw.  Every carrier
 * element is the fp32 value the plain entry point computes, rounded once to nearest even (a NaN stays a NaN).
 * Each pair of entry points (plain, _bf16) is one checked launcher in vit.hip, and the plain form is the _bf16 form without
 * a carrier: the same argument rules (but pl_vit_gelu_* take any element count n, the _bf16 forms rows and cols), and a NULL
 * carrier launches exactly the plain form's kernel.  Without a carrier the fp32 output (y, dx, o, dqkv, du) is required;
 * with one it may be NULL (not written).
 *   pl_vit_ln_fwd_bf16   : y_bf16 = carrier of y (nnorm >= 1)
 *   pl_vit_ln_bwd_bf16   : dx_bf16 = carrier of dx
 *   pl_vit_attn_fwd_bf16 : o_bf16 [rows_pad][heads*64], T = B * seq
 *   pl_vit_attn_bwd_bf16 : dqkv_bf16 [rows_pad][3*heads*64]
 *   pl_vit_gelu_*_bf16   : u, dy, y, du as [rows][cols] (cols % 4 == 0); y_bf16 / du_bf16 their carriers
 *   pl_vit_bf16_pack     : out = carrier of x [rows][cols] (cols % 4 == 0, x 16-byte aligned) */
int pl_vit_ln_fwd_bf16(const float* x, const float* add, int64_t T, int H, int nnorm, const float* g1, const float* b1,
                       const float* g2, const float* b2, float eps, float* x_out, float* y, void* y_bf16, int64_t rows_pad,
                       float* stats, void* stream);
int pl_vit_ln_bwd_bf16(const float* dy, const float* dres, const float* x, const float* stats, int64_t T, int H, int nnorm,
                       const float* g1, const float* b1, const float* g2, float* dx, void* dx_bf16, int64_t rows_pad,
                       float* dgb, void* scratch, void* stream);
int pl_vit_attn_fwd_bf16(const float* qkv, int64_t B, int seq, int heads, int dim_head, float scale, float* o, void* o_bf16,
                         int64_t rows_pad, float* lse, void* stream);
int pl_vit_attn_bwd_bf16(const float* qkv, const float* lse, const float* dout, int64_t B, int seq, int heads, int dim_head,
                         float scale, float* dqkv, void* dqkv_bf16, int64_t rows_pad, void* stream);
int pl_vit_gelu_fwd_bf16(const float* u, int64_t rows, int64_t cols, int64_t rows_pad, float* y, void* y_bf16, void* stream);
int pl_vit_gelu_bwd_bf16(const float* u, const float* dy, int64_t rows, int64_t cols, int64_t rows_pad, float* du,
                         void* du_bf16, void* stream);
int pl_vit_bf16_pack(const float* x, int64_t rows, int64_t cols, int64_t rows_pad, void* out, void* stream);

/* ---- measurement hook (bench.py; not part of the reference interface) ------------------ */
/* While enabled (on = n > 0), every n-th GEMM launch (n = 1: every one) is bracketed by two HIP events
 * recorded on the launch stream -- a pair costs ~2.5 us of stream time, so bench.py samples every 7th launch
 * of its timed region rather than all of them.  pl_prof_read waits for them and sums the durations of the launches whose
 * algorithmic work (2*M*N*K, summed over both problems of a dual launch) lies in
 * [min_flops, max_flops].  Enabling resets the record.  Not capturable. */
int pl_prof_enable(int on);
int pl_prof_read(double min_flops, double max_flops, double* ms_total, int64_t* launches,
                 double* flops_total);

#ifdef __cplusplus
}
#endif
#endif /* POSELIFT_H_ */
