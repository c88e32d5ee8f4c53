// Internal declarations shared by the HIP translation units of libposelift.so.
// gfx950 (MI355X) only: 64-lane wavefronts, MFMA, 160 KB LDS per CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/poselift.h"
#include "adamw.h"
#include "philox.h"
#include "pose_criterion.h"

namespace pl {

constexpr int kWave = 64;
// ReLU as torch computes it, the one form every kernel uses: a NaN stays a NaN (fmaxf returns the other operand, and
// `v > 0 ? v : 0` takes a NaN for "off").  relu_f is IEEE 754-2019 maximum(v, +0) -- one v_maximum3_f32 on gfx950, where
// fmaxf is a canonicalising v_max plus the v_max -- and gives finite v the bits fmaxf(v, 0.f) gave, -0.0f -> +0.0f included.
// relu_on is the matching bitmap / gradient decision: the gradient passes where the input is positive OR NaN (torch's
// threshold_backward).
__device__ __forceinline__ bool relu_on(float v) { return !(v <= 0.f); }
__device__ __forceinline__ float relu_f(float v) { return __builtin_elementwise_maximum(v, 0.f); }
// the same maximum between two values: a NaN on either side wins (max-pool's window maximum)
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// template arguments chosen at run time travel to the one launch site of a kernel template as values of these types
template <bool V> using Bool = std::integral_constant<bool, V>;
template <int V> using Int = std::integral_constant<int, V>;

void set_error(const char* fmt, ...);

#define PL_FAIL(code, ...)        \
  do {                            \
    ::pl::set_error(__VA_ARGS__); \
    return (code);                \
  } while (0)

#define PL_CHECK_LAUNCH(what)                                              \
  do {                                                                     \
    hipError_t e__ = hipGetLastError();                                    \
    if (e__ != hipSuccess)                                                 \
      PL_FAIL(PL_EHIP, "%s: launch failed: %s", what, hipGetErrorString(e__)); \
  } while (0)

// The alignment contract of caller pointers: an entry point refuses, before any launch, a caller's pointer that a
// kernel behind it reads or writes wider than 4 bytes and that is not 16-byte aligned.  NULL (an optional pointer) passes.
#define PL_REQUIRE_ALIGNED16(who, ptr)                                       \
  do {                                                                       \
    if (reinterpret_cast<uintptr_t>(ptr) & 15)                               \
      PL_FAIL(PL_EINVAL, "%s: %s not 16-byte aligned", who, #ptr);           \
  } while (0)

#define PL_TRY(expr)        \
  do {                      \
    int rc__ = (expr);      \
    if (rc__ != PL_OK) return rc__; \
  } while (0)

// ---------------------------------------------------------------------------------
// fp32 MFMA GEMM  (gemm_f32.hip)
// ---------------------------------------------------------------------------------
enum GemmLayout { kNT = 0, kNN = 1, kTN = 2 };

struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  int M, N, K;
  int lda, ldb, ldc;
  int split_k;              // >1: slice z writes C + z*M*ldc (slab), no epilogue extras
  // epilogue (all optional)
  const float* bias;        // [N]     v += bias[col]
  const float* addend;      // [M][ldc] v += addend[row][col]   (may alias C)
  float* stat_sum;          // [2*ceil(M/128)][N] per-64-row-group column sums of v
  float* stat_m2;           //   ... and sums of squares about the group mean
  const float* col_scale;   // [N]     v = v*scale[col] + shift[col]  (eval-mode BN fold)
  const float* col_shift;
  int relu;                 // 1: v = max(v, 0) before the resid add; 2: after it (Bottleneck order)
  const float* resid;       // [M][ldc] v += resid[row][col] after relu (may alias C)
  int arith;                // a GemmArith value (below)
  // Implicit-GEMM convolution (launch_conv_nhwc only; conv_cin == 0 otherwise): A is not a matrix but the
  // NHWC input x [B][H][W][Cin]; row m = (b, oh, ow), k = (kh*KW + kw)*Cin + ci, element
  // x[b][oh*stride - pad + kh][ow*stride - pad + kw][ci] or 0 outside the image.  B = weights [N][K] (OHWI).
  int conv_cin, conv_h, conv_w, conv_ho, conv_wo, conv_kw, conv_stride, conv_pad_h, conv_pad_w;
  int conv_stride_w;        // planes convolutions: stride along w when it differs from conv_stride (along h); 0 = the same
  // BatchNorm-backward pass 1 of the layer BELOW, folded into the epilogue of the dX GEMM that produces its incoming
  // gradient (planes GEMM only; bnr_z == NULL otherwise): C is g = d(act of that layer); with its saved z, ReLU/dropout
  // bitmap, batch mean and rstd the epilogue also emits, per 64-row block and column, sum dy and sum dy*zhat
  // (dy = g * bit * bnr_kscale) -- [M/64][N] each -- and per (64-row block, 64-column block) max |dy| and max |zhat|.
  const float* bnr_z;
  const uint64_t* bnr_bits;
  const float* bnr_mean;
  const float* bnr_rstd;
  float bnr_kscale;
  float* bnr_part_dy;       // [M/64][N]
  float* bnr_part_dyz;      // [M/64][N]
  float* bnr_amax;          // [(M/64) * (N/64)][2] or NULL
  // planes GEMM (staged epilogue): the result ALSO (C != NULL) or ONLY (C == NULL) as operand planes of the next GEMM --
  // cpl_kind 0 none, 1 one bf16 plane, 2 fp16 pair (h, l) of cpl_scale * value; addressed like C (row * ldc + col)
  unsigned short* cpl_h; unsigned short* cpl_l; float cpl_scale; int cpl_kind;
  uint32_t* cpl_range; int cpl_site;      // range guard of those planes (PlaneOut::range / site)
  // planes convolution launches only: row m = (b, a, c) of a conv_ho x conv_wo grid is stored at pixel
  // (b, 2a + scat_ph, 2c + scat_pw) of a [B][2 conv_ho][2 conv_wo][ldc] map (one output parity of a 4x4 stride-2
  // transposed convolution); plain stores only
  int scat_on, scat_ph, scat_pw;
  // host side only: scratch for the small-batch split-K path (gemm_thin.hip); NULL = never take it
  float* thin_scratch;
  size_t thin_scratch_floats;
};

// GemmArgs::arith.  0-2 are the PLDtype values; launch_gemm_f32 runs every problem that is not whole tiles, and an
// kArithBf16Planes problem that misses that pipeline's conditions, in exact fp32 (f32_route, gemm_f32.hip).
enum GemmArith : int {
  kArithF32 = 0,            // fp32 MFMA
  kArithBf16 = 1,           // PL_BF16: operands rounded to bf16 on the way to the MFMA
  kArithX6 = 2,             // PL_BF16X6: three-way bf16 split, six MFMAs, fp32-grade products; the library picks the main loop
  kArithX6Planes = 5,       //   ... forced to the planes loop (test hook of pl_gemm_arith)
  kArithX6Frag = 6,         //   ... forced to the fragment-split loop (test hook of pl_gemm_arith)
  kArithBf16Planes = 7,     // PL_BF16 on the planes pipeline: the conv path's NT GEMMs (conv.hip)
};

// y = conv2d(x, w) as an implicit GEMM on the PL_BF16X6 planes pipeline; a.A = x, a.B = w [Cout][KH*KW*Cin],
// a.M = B*Ho*Wo, a.N = Cout, a.K = KH*KW*Cin and the conv_* fields filled in; whole tiles only.
int launch_conv_nhwc(const GemmArgs& a, hipStream_t s);
// four independent convolutions of identical shape (the four output parities of a stride-2 transposed
// convolution) in ONE launch: at 8x8 / 16x16 input maps a single one fills a quarter of the CUs
int launch_conv_nhwc_group4(const GemmArgs* a, hipStream_t s);
// weight gradient of a convolution: the TN planes GEMM over pixels with the B operand gathered from x
int launch_conv_wgrad(const GemmArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------
// planes GEMM (gemm_planes.hip / gemm_planes.h): operands pre-split into 16-bit planes by their producers
// ---------------------------------------------------------------------------------
// Where a streaming kernel writes the planes of the tensor it produces ([rows][cols] row-major, like the tensor):
//   kind 0 none; 1 one bf16 plane (PL_BF16 storage); 2 fp16 pair (PL_F16X3): h = fp16(S x), l = fp16((S x - h) * 2048)
// S = scale, or -- dyn != NULL -- the device value dyn[0] (a power of two written by an earlier kernel).
struct PlaneOut {
  unsigned short* h;
  unsigned short* l;
  float scale;
  const float* dyn;
  int kind;
  int nt;             // the tensor (planes and its fp32 twin) leaves with nontemporal stores: far larger than the caches
  uint32_t* range;    // range guard (static scales, kind 2): the caller's record or NULL, and this writer's slot in it
  int site;
};
// The range guard's record for launches enqueued by this thread (pl_range_monitor; NULL = none), and a static-scale PlaneOut
// joined to it: fp16 planes only, and never planes scaled on the device.
uint32_t* range_record();
inline int range_site_act(int layer) { return PL_RANGE_SITE_LIFTER_ACT + (layer < 7 ? layer : 7); }
inline void range_watch(PlaneOut& po, int site) {
  if (po.kind == 2 && !po.dyn) { po.range = range_record(); po.site = site; }
}
// outputs at least this large are streamed past the caches (their consumer reads them from HBM whatever the store policy)
constexpr long long kNontemporalBytes = 64ll << 20;
constexpr float kActPlaneScale = 1.0f;      // activations: fp16 covers 6e-5 .. 65504 in h, the remainder in l
constexpr float kWeightPlaneScale = 16.0f;  // weights (|w| ~ 0.03 at init): 3.8e-6 .. 4094
// conv path: eval-mode feature maps of an unnormalised network reach 1e5 (seeded test weights: 6.7e4 after the first
// transposed convolution) -- 1/64 keeps h finite up to 4.2e6; below |x| = 4e-3 h goes subnormal and l carries the value to
// an absolute 1e-9 (relative 2^-22 above)
constexpr float kConvActPlaneScale = 1.0f / 64.0f;

struct PlanesGemmArgs {
  GemmArgs e;                 // M, N, K, C, ldc, split_k and the epilogue fields (A, B, lda, ldb, arith unused)
  const unsigned short* A;    // planes of A: k-contiguous [M][K] (NT, NN) or k-strided [K][M] (TN)
  const unsigned short* B;    // planes of B: k-contiguous [N][K] (NT) or k-strided [K][N] (NN, TN)
  int64_t a_plane, b_plane;   // elements between two planes of one tensor
  int lda, ldb;               // row strides (elements) of the plane matrices
  int mode;                   // plp::PlanesMode: 0 bf16 (one plane), 2 f16x3 (two planes)
  float out_scale;            // acc * out_scale [* dyn_inv[0]] before the epilogue: 1 / (S_A S_B)
  const float* dyn_inv;       // device scalar or NULL
};
bool planes_gemm_ok(GemmLayout layout, const PlanesGemmArgs& a);
// What launch_gemm_planes runs for a problem planes_gemm_ok accepted on a device of ncu CUs (the table: DESIGN 3a): the
// kernel family, its form and its grid.  A plain function of its arguments.
enum class PlanesFamily { OneItem, Persistent, Wide, T64 };
struct PlanesRoute {
  PlanesFamily family;
  bool persist;               // one workgroup per CU walks nwork items (else one item per workgroup)
  bool edge;                  // overhanging tiles or a gathered operand: guarded loads and stores
  int conv;                   // 0 none, 1 A gathered as a convolution input (NT), 2 B gathered, weight gradient (TN)
  int grid, nwork;
};
PlanesRoute planes_route(GemmLayout layout, const PlanesGemmArgs& a, int ncu);
int launch_gemm_planes(GemmLayout layout, const PlanesGemmArgs& a, hipStream_t s);
// dX = dz W (NN) and dW = dz^T a (TN, split-K slabs) of one layer in ONE launch.  `sum` (or NULL): a split-K sum of another
// layer that the launch carries on its loader waves -- out[n] = the slabs part + r n, r < slabs, added in slab order, with
// the arithmetic of launch_reduce_rows_multi's kind-1 job; nothing else may touch part or out while the launch runs.  Ask
// planes_pair_carries_slab_sum first: a sum the launch cannot carry is an error.
struct SlabSum { const float* part; float* out; int slabs; int64_t n; };
bool planes_pair_carries_slab_sum(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn, int slabs, int64_t n);
int launch_gemm_planes_pair(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn, const SlabSum* sum, hipStream_t s);

int launch_gemm_f32(GemmLayout layout, const GemmArgs& a, hipStream_t s);
// M <= kThinGemmMaxM rows (NT, NN): the contraction split over the chip, exact fp32 MFMA, slabs + one reduce/epilogue
// launch (gemm_thin.hip) on a.thin_scratch; launch_gemm_f32 takes it for problems that are not whole tiles when that is set
constexpr int kThinGemmMaxM = 512;
bool thin_gemm_ok(GemmLayout layout, const GemmArgs& a);
size_t thin_gemm_scratch_floats(int M, int N, int K);
int launch_gemm_thin(GemmLayout layout, const GemmArgs& a, hipStream_t s);
int launch_gemm_f32_pair(const GemmArgs& nn, const GemmArgs& tn, hipStream_t s);
int gemm_stat_groups(int M);  // number of 64-row groups the stats epilogue emits
int prof_enable(int on);
void* prof_begin_flops(double flops, hipStream_t s);   // NULL when this launch is not sampled
void prof_end(void* rec, hipStream_t s);
int prof_read(double min_flops, double max_flops, double* ms_total, int64_t* launches, double* flops_total);

// ---------------------------------------------------------------------------------
// streaming kernels: BatchNorm (batchnorm.hip)
// ---------------------------------------------------------------------------------
inline int bitmap_words_per_row(int H) { return ((H + 255) / 256) * 4; }

// A BatchNorm layer's parameters and running statistics (built once per layer: layer_of() in api.hip, the C ABI's
// arguments on the conv path).  running_mean / running_var / batches may be NULL (nothing to update).
struct BnParams {
  const float *gamma, *beta;
  float eps, momentum;
  float *running_mean, *running_var;
  int64_t* batches;
};
// What a layer's forward saves for its backward: the pre-activation, the ReLU & keep bitmap and the batch statistics.
// tile_bits: the bitmap is in the tile format of small_layer.hip (the layer's forward ran there) instead of the row format
// of bn_apply_row.
struct BnSaved {
  float* z;
  uint64_t* bits;
  float *mean, *rstd;
  bool tile_bits;
};

// BN statistics: merge per-group (sum, M2) partials -> mean/rstd/scale/shift, update running
// (stat = [world][2][G][H]: per rank G rows of sums then G rows of M2 over group_rows rows each; B = rows per rank)
struct BnFinalizeArgs {
  const float* stat;
  int G, group_rows, world, B, H;
  BnParams bn;
  float *mean, *rstd, *scale, *shift;
};
int launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t s);

// act = [resid +] dropout(relu(z*scale + shift)); bits = keep&positive bitmap
struct BnApplyArgs {
  const float* z;
  const float *scale, *shift;   // [Hc]; NULL: identity (no BatchNorm); not read when fin.stat is set
  const float* resid;           // optional
  float* act;                   // NULL: planes only
  uint64_t* bits;
  int B, H;
  int Hc;                       // real columns behind the H virtual ones (conv path, bn_colstats_kernel); 0: H
  bool no_relu;                 // BatchNorm alone; the bitmap is all ones
  bool resid_before_relu;       // relu(bn(z) + resid), the Bottleneck's join, instead of resid + relu(bn(z))
  DropKey drop;                 // dropout_key(); dropout_key(0, ...) where there is no dropout
  PlaneOut planes;              // kind != 0: also (act == NULL: only) write the activation as GEMM operand planes
  // fin.stat != NULL: the statistics finalize (launch_bn_finalize's job) inside this launch.  The kernel takes local
  // statistics (world, scale and shift are not read; B and H are this launch's) of at most 16 groups; plan() routes
  // single-process layers of at most 4 groups (256 rows) here (Stats::InApply).
  BnFinalizeArgs fin;
};
int launch_bn_apply(const BnApplyArgs& a, hipStream_t s);

int bwd_row_chunks(int B, int H);
// pass 1: partial column sums of dy and dy*zhat, dy = g * bits * keep_scale
struct BnBwdReduceArgs {
  const float* g;
  BnSaved saved;
  float keep_scale;
  int B, H;
  int Hc;                       // 0: H
  int rc;                       // row chunks (grid.y); 0: bwd_row_chunks(B, H)
  float *part_dy, *part_dyz;
  float* part_amax;             // optional: [strips * rc][2] per-workgroup maxima of |dy| and |zhat| (the dz range bound, below)
  const float* join_g2;         // the residual join's backward: g := (g + join_g2 (or 0)) where the bitmap is set, written
  float* join_dx;               //   to join_dx by this pass (NULL: none)
};
int launch_bn_bwd_reduce(const BnBwdReduceArgs& a, hipStream_t s);

// dz_scale (optional, with part_amax of n_amax workgroups): {S, 1/S}, S the power of two that maps the bound
// max|c0| max|dy| (2 + max|zhat|) >= max|dz| to at most 2^14 (fp16 planes of dz, PL_F16X3)
struct BnBwdFinalizeArgs {
  const float* part;
  int RC, world, rank, B, H;
  const float *gamma, *rstd;
  float *coef, *dgamma, *dbeta;
  const float* part_amax;
  int n_amax;
  float* dz_scale;
  int eval_mode;
  int64_t rstride;
  int amax_world;               // 0: 1
};
int launch_bn_bwd_finalize(const BnBwdFinalizeArgs& a, hipStream_t s);
// pass 2: dz = c0*(dy - c1 - zhat*c2)  (bn) or dz = dy (no bn); partial column sums of dz
struct BnBwdDzArgs {
  const float* g;
  BnSaved saved;
  const float* coef;
  float keep_scale;
  int bn, B, H;
  int Hc;                       // 0: H
  int rc;                       // row chunks (grid.y); 0: bwd_row_chunks(B, H)
  float* dz;                    // NULL: planes only
  float* part_db;
  PlaneOut planes;              // kind != 0: also write dz as GEMM operand planes
};
int launch_bn_bwd_dz(const BnBwdDzArgs& a, hipStream_t s);
// eval-mode fold: scale = gamma*rsqrt(rv+eps), shift = (bias - rm)*scale + beta  (bn) or 1, bias
int launch_bn_fold_eval(const float* bias, const BnParams* bn, int H, float* scale, float* shift, hipStream_t s);
// eval-mode BatchNorm for the saved-state forward: mean := running mean, rstd := rsqrt(running var + eps), scale, shift
// (reads a.bn, a.H and the four outputs)
int launch_bn_eval_stats(const BnFinalizeArgs& a, hipStream_t s);
// Small batches (B <= kBnSmallRows, local statistics, fp32 outputs): statistics + finalize + apply of a hidden layer in ONE
// launch (a workgroup owns a 256-column strip for all rows, held in registers), and pass 1 + finalize + dz + bias gradient
// of its backward.  Measured same-box (bench.py --batch B): B = 64 0.305 -> 0.280 ms per step; B = 100 / 127 with sixteen
// rows per wave 0.42 / 0.45 -> 0.47 / 0.52 ms (slower: kept to 64 rows).
constexpr int kBnSmallRows = 64;
struct BnSmallFwdArgs {
  BnSaved saved;                // z read; bits, mean, rstd written (row-format bitmap)
  BnParams bn;
  const float* resid;           // optional
  float* act;
  int B, H;
  DropKey drop;
};
int launch_bn_small_fwd(const BnSmallFwdArgs& a, hipStream_t s);
// what the BatchNorm backward of a small-batch layer reads and writes (besides its incoming gradient and dz)
struct SmallBnLayer {
  BnSaved saved;
  const float* gamma;
  float *dgamma, *dbeta, *dbias;
};
struct BnSmallBwdArgs {
  const float* g;
  SmallBnLayer layer;
  float keep_scale;
  int B, H;
  float* dz;
};
int launch_bn_small_bwd(const BnSmallBwdArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------
// streaming kernels: fixed-order sums (reduce.hip)
// ---------------------------------------------------------------------------------
// out[i] = sum_s slabs[s*n + i]
int launch_reduce_slabs(const float* slabs, int nslab, int64_t n, float* out, hipStream_t s);
// njobs independent out[c] = sum_r part[r][c] reductions in one launch
// kind 2 (at most one job): out[0] = (sum of the R MSE partials) * loss_inv_n, then loss_tick[0] += 1 -- mse_final_kernel
struct RowJob {
  const float* part;
  float* out;
  int R, H, kind, transK;
};
int launch_reduce_rows_multi(const RowJob* jobs, int njobs, float loss_inv_n, uint64_t* loss_tick, hipStream_t s);
// out[r][c] = bias[c] + sum_s slabs[s][r][c]
int launch_reduce_slabs_bias(const float* slabs, int nslab, int rows, int cols, const float* bias,
                             float* out, hipStream_t s);
// partial column sums of X[rows][cols] -> part[RC][cols], RC = colsum_chunks(rows)
int colsum_chunks(int rows);
int launch_colsum_partial(const float* X, int rows, int cols, float* part, hipStream_t s);
int launch_fill(float* p, int64_t n, float v, hipStream_t s);

// ---------------------------------------------------------------------------------
// streaming kernels: operand planes of a tensor no producer kernel splits (planes_split.hip)
// ---------------------------------------------------------------------------------
// x [n] fp32 -> planes (static scale); n % 4 == 0, 16-byte aligned
int launch_split_planes(const float* x, int64_t n, const PlaneOut& out, hipStream_t s);
// PlaneOut of a caller's planes buffer ([2][n] fp16 for PL_F16X3, [n] bf16 for PL_BF16; NULL -> kind 0)
int plane_out_of(int mode, void* planes, int64_t n, float scale, const float* dyn, PlaneOut* po, const char* who);

// ---------------------------------------------------------------------------------
// streaming kernels: the train criterion (criterion.hip)
// ---------------------------------------------------------------------------------
// pl_pose_loss_fwd_bwd (pl_mse_fwd_bwd: Crit{}, B = 1, O = n) + (tick != NULL) tick[0] += 1 once the loss is written
// (PLDesc.step_dev, graph replay)
int loss_fwd_bwd_tick(const float* pred, const float* tgt, int64_t B, int64_t O, const Crit& c, float grad_scale, float* dpred,
                      float* loss_out, void* scratch, uint64_t* tick, void* stream, const char* who);
int loss_partial_only(const float* pred, const float* tgt, int64_t B, int64_t O, const Crit& c, float grad_scale, float* dpred,
                      void* scratch, void* stream, const char* who);
int loss_partials(const Crit& c, int64_t B, int64_t O);
// the output Linear's slab reduce folded into the loss partial pass (fused train step; bit-identical to the two launches)
bool mse_from_slabs_supported(int splits, int N);
int loss_partial_from_slabs(const float* part, int splits, int B, int N, const float* bias, const float* tgt, const Crit& c,
                            float grad_scale, float* y, float* dpred, void* scratch, void* stream);

// ---------------------------------------------------------------------------------
// streaming kernels: the flat optimizer (optim.hip)
// ---------------------------------------------------------------------------------
// the flat AdamW step over p, g, m, v [n] (adamw_kernel's only launch site).  in: the kernel's own argument block (adamw.h);
// lr_dev / t_dev, the plane fields (adamw_planes) and the clip record are the optional parts, zero when absent
struct AdamWArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  AdamWIn in;
  const PLEma* ema;             // optional: the averaged weights follow in the same launch (e: beside p, for the same [n])
};
int launch_adamw(const AdamWArgs& a, hipStream_t s);
int check_ema(const PLEma& ema, const char* who);

// ---------------------------------------------------------------------------------
// streaming kernels: the pose feed (pose_feed.hip)
// ---------------------------------------------------------------------------------
// the checks of a PLPoseAug's parameters (fn: the entry point named in the message) and the plan the transforms of
// pose_augment.h and frame_warp.h read
namespace pa { struct Plan; }
int pose_aug_plan(const char* fn, const PLPoseAug* aug, uint64_t epoch, pa::Plan* plan);
// the checks of a PLPoseCrop (and of the flip of the PLPoseAug that goes with it, nullable) and the spec frame_crop.h reads
namespace fc { struct Spec; }
int crop_spec(const char* fn, const PLPoseCrop* crop, const PLPoseAug* aug, fc::Spec* spec);

// ---------------------------------------------------------------------------------
// small batches (small_layer.hip)
// ---------------------------------------------------------------------------------
// Small batches, hidden layers behind the first (small_layer.hip): a workgroup owns 16 columns for all B <= 64 rows, so one
// launch is Linear + BatchNorm1d (batch statistics) + ReLU + Dropout (+ skip) forward, and one launch is dX = dz W (+ skip
// gradient) followed by the BatchNorm backward of the layer below.  Their ReLU & keep bitmap is in the "tile format" of
// small_layer.hip (tile_bits above: bn_small_bwd reading such a layer).
bool small_layer_ok(int B, int H, int K);
// ... the first layer (K = in_dim <= 256 inputs: contraction on the vector unit) forward, its weight gradient in the backward
// launch of the layer above, and the whole top of the backward pass (g = dy W2, BatchNorm backward of the last hidden layer,
// dW2, db2; out_dim <= 64) as one launch.
bool small_first_ok(int K);
bool small_top_ok(int O);
// One hidden layer of a small batch, forward.  launch_small_layer_fwd (training: B <= 64 rows, batch statistics) reads every
// field; launch_small_layer_eval (any B; running statistics, Dropout the identity, nothing saved) ignores saved and drop.
struct SmallLayerFwdArgs {
  const float *a, *W, *bias;
  BnParams bn;
  BnSaved saved;                // z, bits (tile format), mean, rstd: written
  const float* resid;           // optional
  float* act;
  int B, H, K, layer;
  DropKey drop;
  bool first;                   // the first layer (K = in_dim <= 256 inputs: contraction on the vector unit)
  // ypart != NULL (the last hidden layer of a fused train step / of an evaluation): the launch also leaves its share of the
  // output Linear, ypart [H / 16][B][64] (columns < O); launch_small_mse adds the slabs up: y, dpred = grad_scale * 2 (y - t)
  // / (B O) and small_mse_partials(B, O) partial sums of (y - t)^2 -- no launch for the output layer, none for its slab
  // reduce; an evaluation hands them to launch_small_out
  const float* W2;
  float* ypart;
  int O;
  // a_planes (PL_F16X3 descriptors, not the first layer): the input as two fp16 planes [B][K] (h, l) -- the contraction then
  // runs as three fp16 MFMAs per product (fp32-grade, a fifth of the MFMA time of the exact fp32 form); out_planes: the output
  // also as planes [B][H], for the next layer's launch
  const unsigned short* a_planes;
  unsigned short* out_planes;
};
int launch_small_layer_fwd(const SmallLayerFwdArgs& a, hipStream_t s);
// evaluation forward (model.eval()): the same layer kernels with the BatchNorm fold on the running statistics as tail, the
// grid also over 64-row blocks (any B; every row the same bits whatever the batch), and launch_small_out for the output layer
int launch_small_layer_eval(const SmallLayerFwdArgs& a, hipStream_t s);
// the output Linear from the NS slabs the last hidden layer's launch left: y = bias + their sum (launch_small_out reads
// these fields alone) and, launch_small_mse, dpred = grad_scale * 2 (y - tgt) / (B O) and the MSE partials in mpart
// (crit: the criterion in MSE's place; its partials: small_loss_partials)
struct SmallHeadArgs {
  const float* ypart;
  int NS, B, O;
  const float* bias;
  float* y;
  const float* tgt;
  float grad_scale;
  float *dpred, *mpart;
  Crit crit;
};
int launch_small_out(const SmallHeadArgs& a, hipStream_t s);
// the Linear alone with the statistics partials of a tile GEMM's epilogue, for TRAINING batches of 65 ... 512 rows: the tile
// GEMMs have 8 ... 32 tiles for 256 CUs there (22 us per forward GEMM at any of these sizes; this form: 9-17 us)
// (a_planes != NULL: the input as fp16 planes [M][K] (h, l) instead of a; stat_sum / stat_m2 [groups][H], optional)
struct SmallLinearStatsArgs {
  const float* a;
  const unsigned short* a_planes;
  const float *W, *bias;
  float* z;
  int M, H, K;
  float *stat_sum, *stat_m2;
  int groups;
};
int launch_small_linear_stats(const SmallLinearStatsArgs& a, hipStream_t s);
int small_mse_partials(int B, int O);     // partial sums launch_small_mse leaves in mpart (<= 64)
int small_loss_partials(const Crit& c, int B, int O);      // ... with a criterion: the grouped kind counts 64 joints a workgroup
int launch_small_mse(const SmallHeadArgs& a, hipStream_t s);
// g = dz W (+ addend) -> gout (or NULL), then the BatchNorm backward of the layer below -> dz_lo
struct SmallLayerBwdArgs {
  const float *dz, *W;
  const float* addend;          // optional
  float* gout;                  // optional
  int B, H, K;
  SmallBnLayer below;
  float kscale;
  float* dz_lo;
  const float* a_in;            // dW != NULL: + dW = dz^T a_in (extra workgroups)
  float* dW;
  const float* x1;              // dW1 != NULL: the layer below is the first one, + dW1 = dz_lo^T x1 (K1 inputs)
  float* dW1;
  int K1;
  const struct AdamWRide* adam; // optional: a slice of the AdamW step on spare workgroups (adamw.h)
  const PLEma* ema;             // optional, with adam: that slice's averaged weights (e: the slice's, beside adam->p)
};
int launch_small_layer_bwd(const SmallLayerBwdArgs& a, hipStream_t s);
// the whole top of the backward pass: g = dy W2 -> gout, the BatchNorm backward of the last hidden layer -> dz_top, dW2, db2
struct SmallTopBwdArgs {
  const float *dy, *W2, *h;
  int B, H, O;
  float *gout, *dW2, *db2;
  SmallBnLayer top;
  float kscale;
  float* dz_top;
  const float* mpart;           // loss != NULL: + loss = inv_n * sum of the np partials in mpart, tick[0] += 1
  int np;
  float inv_n;
  float* loss;
  uint64_t* tick;
};
int launch_small_top_bwd(const SmallTopBwdArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------
// skinny layers (skinny.hip): 34 -> H and H -> 51, MFMA straight from registers
// ---------------------------------------------------------------------------------
bool skinny_supported(int K, int H);           // narrow dimension specialised (34, 51), H % 128 == 0
int skinny_chunks(int B);                      // row tasks (64 rows each)
int skinny_stat_groups(int B);                 // 64-row BN statistics groups it emits
// BatchNorm-backward pass 1 of the layer that consumes a kernel's output as its incoming gradient, done on the block just
// produced (GemmArgs::bnr_* for the planes GEMM); z == NULL: none
struct BnrEpilogue {
  const float* z;
  const uint64_t* bits;
  const float *mean, *rstd;
  float kscale;
  float *part_dy, *part_dyz;  // [B/64][H]
  float* amax;                // optional: per (64-row group, column strip) max |dy| and max |zhat|
};
// out [B][H] = X [B][K] W^T + bias (the input layer's forward: W [H][K], stat_sum / stat_m2 optional) or, w_transposed,
// X W (g = dy W5: W [K][H], no bias; bnr: 32-column strips, whole groups only)
struct SkinnyWideOutArgs {
  const float *X, *W, *bias;
  float* out;
  int B, K, H;
  bool w_transposed;
  float *stat_sum, *stat_m2;
  BnrEpilogue bnr;
};
int launch_skinny_wide_out(const SkinnyWideOutArgs& a, hipStream_t s);
// X^T D, X [B][K], D [B][H]: partials in part (skinny_in_chunks(B) x K x H floats), then -- reduce -- their sum in out, [K][H]
// or, out_transposed, [H][K].  Without reduce the caller combines them (launch_reduce_rows_multi: R = skinny_in_chunks(B),
// H = K*H, transK = K for the transposed form) and out is not touched
struct SkinnyWideInArgs {
  const float *X, *D;
  int B, K, H;
  float* part;
  bool reduce, out_transposed;
  float* out;
  float* xsum;                // optional: skinny_in_chunks(B) x K partial column sums of X (the output layer's bias gradient:
                              // X = dy), to be combined like any other partial (R = skinny_in_chunks(B), H = K)
};
int launch_skinny_wide_in(const SkinnyWideInArgs& a, hipStream_t s);
int skinny_in_chunks(int B);
bool skinny_narrow_out_supported(int H, int N);
size_t skinny_narrow_out_part_floats(int B, int H);
// part: [splits][B][64] slabs of h W^T, then -- reduce -- y = bias + their sum; without reduce that is left to the caller
// (mse_partial_from_slabs)
struct SkinnyNarrowOutArgs {
  const float *h, *W;
  int B, H, N;
  float* part;
  bool reduce;
  const float* bias;
  float* y;
};
int launch_skinny_narrow_out(const SkinnyNarrowOutArgs& a, hipStream_t s);
int skinny_narrow_out_splits(int B, int H);

}  // namespace pl
