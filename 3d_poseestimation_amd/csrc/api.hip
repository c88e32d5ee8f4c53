// C ABI of libposelift.so: arena layout, workspace plan and the forward / backward
// launch sequences of the lifter (include/poselift.h).  Host code only; every kernel
// lives in the kernel files (gemm_*.hip, batchnorm.hip, reduce.hip, criterion.hip, optim.hip, ...).
//
// Layer numbering used everywhere: hidden layer 0 is LinearModel.w1/batch_norm1
// (baselineModel.py:67-68,90-94); residual block s owns hidden layers 1+2s (its w1) and
// 2+2s (its w2) (baselineModel.py:23-27,33-45); "final" is LinearModel.w2 (:77,100).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "adamw.h"
#include "pl_internal.h"

namespace pl {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

int check_desc(const PLDesc* d, bool need_arenas) {
  if (!d) PL_FAIL(PL_EINVAL, "descriptor is NULL");
  if (d->in_dim <= 0 || d->out_dim <= 0 || d->hidden <= 0 || d->num_stage < 0)
    PL_FAIL(PL_ESHAPE, "bad dims in=%d hidden=%d out=%d stages=%d", d->in_dim, d->hidden, d->out_dim, d->num_stage);
  if (d->hidden % 4 != 0) PL_FAIL(PL_ESHAPE, "hidden=%d must be a multiple of 4", d->hidden);
  if (d->dtype != PL_F32 && d->dtype != PL_BF16 && d->dtype != PL_BF16X6 && d->dtype != PL_F16X3)
    PL_FAIL(PL_EDTYPE, "dtype %d is not a PLDtype", d->dtype);
  if (!(d->p_dropout >= 0.f && d->p_dropout <= 1.f)) PL_FAIL(PL_EINVAL, "p_dropout=%f outside [0,1]", d->p_dropout);
  if (need_arenas) {
    if (!d->params) PL_FAIL(PL_EINVAL, "params arena is NULL");
    if (reinterpret_cast<uintptr_t>(d->params) & 15) PL_FAIL(PL_EINVAL, "params arena not 16-byte aligned");
    if (d->bn && !d->bn_running) PL_FAIL(PL_EINVAL, "bn_running arena is NULL");
  }
  if (d->sync) {
    const PLSync* y = d->sync;
    if (y->world < 1 || y->rank < 0 || y->rank >= y->world)
      PL_FAIL(PL_EINVAL, "PLSync: rank %d of world %d", y->rank, y->world);
    if (y->world > 1 && !y->gather) PL_FAIL(PL_EINVAL, "PLSync: gather callback is NULL");
  }
  return PL_OK;
}

// cross-rank BatchNorm statistics (PLSync): world 1 = local statistics
inline int sync_world(const PLDesc* d) { return (d->sync && d->bn) ? d->sync->world : 1; }
inline int sync_rank(const PLDesc* d) { return (d->sync && d->bn) ? d->sync->rank : 0; }

// Partial-statistics buffer: [world][2][P][H] floats; rank r's slab holds its P partial rows of the
// first quantity then P rows of the second.  The finalize kernels walk all world*P partials.
int sync_gather(const PLDesc* d, float* base, int64_t floats_per_rank, hipStream_t s) {
  if (sync_world(d) <= 1) return PL_OK;
  const int rc = d->sync->gather(d->sync->user, base, floats_per_rank, (void*)s);
  if (rc != 0) PL_FAIL(PL_ESYNC, "PLSync gather callback failed (%d)", rc);
  return PL_OK;
}

// PL_F16X3: the 1024-wide GEMMs run on fp16 operand planes written by the kernels that produce the tensors
// (gemm_planes.hip).  That path wants whole 128x128 tiles and BatchNorm (its backward pass 1 supplies the range bound
// of dz; under cross-rank statistics every rank's maxima travel in the gathered slab, round 3); anything else runs the
// same fp32-grade arithmetic class on the round-1 kernels (PL_BF16X6: fp32 operands split inside the GEMM) -- never a
// lower precision, never the CPU.
// PL_BF16 takes the same path with ONE bf16 plane per tensor (kind 1): bf16 STORAGE of the GEMM operands
// (activations, dz, weight shadow), no scales -- bf16 has fp32's exponent range.
int tn_splits(int M, int N, int K) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int s = 256 / tiles;
  const int kmax = (K + 127) / 128;
  if (s > kmax) s = kmax;
  return s < 1 ? 1 : s;
}

inline int planes_kind(const PLDesc* d, int64_t B) {       // PlaneOut::kind of the operand planes, 0 = not on that path
  const bool ok = d->bn && d->hidden % 128 == 0 && B % 128 == 0 && d->num_stage >= 1 &&
                  B * (int64_t)d->hidden * 4 < (1ll << 30);
  if (!ok) return 0;
  // the weight-gradient GEMM splits K = B into tn_splits slices of whole 32-k tiles (H = 512 with B = 128 * 17 would
  // not): such a batch runs on the round-1 kernels like every other shape off the tile grid
  if (B % (32 * (int64_t)tn_splits(d->hidden, d->hidden, (int)B)) != 0) return 0;
  return d->dtype == PL_F16X3 ? 2 : (d->dtype == PL_BF16 ? 1 : 0);
}
inline int arith_of(const PLDesc* d) { return d->dtype == PL_F16X3 ? (int)PL_BF16X6 : d->dtype; }

struct ParamLayout {
  int L;                       // hidden layers
  std::vector<int64_t> off, numel;
  int64_t total;
};

ParamLayout param_layout(const PLDesc* d) {
  ParamLayout p;
  p.L = 1 + 2 * d->num_stage;
  int64_t o = 0;
  auto add = [&](int64_t n) {
    p.off.push_back(o);
    p.numel.push_back(n);
    o = align_up(o + n, 64);
  };
  for (int l = 0; l < p.L; ++l) {
    const int64_t fan_in = l == 0 ? d->in_dim : d->hidden;
    add((int64_t)d->hidden * fan_in);
    add(d->hidden);
    add(d->hidden);
    add(d->hidden);
  }
  add((int64_t)d->out_dim * d->hidden);
  add(d->out_dim);
  p.total = o;
  return p;
}

// Output layer y = h W^T + b with N = out_dim (51): only ceil(M/128) tiles, so the K = hidden
// contraction is split over workgroups (slabs) until the chip is full, then reduced with the bias.
int out_splits(int M, int N, int K) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  int s = 256 / tiles;
  const int kmax = K / 128;
  if (s > kmax) s = kmax;
  return s < 1 ? 1 : s;
}

// The route: which kernels run each part of the lifter, decided by plan() from the descriptor and the batch alone -- so
// every call (forward, backward, a cut range of it, the queries) agrees on it and the workspace holds what they touch.  A
// call combines it only with its own arguments; eval_bn (no batch statistics) takes none of the small-batch routes.
enum class Lin : uint8_t {     // forward Linear of a hidden layer when it is a launch of its own (under eval_bn: always)
  Skinny, Planes, Gemm,        // first layer on skinny.hip; the planes tile GEMM; launch_gemm_f32
  // launch_small_linear_stats, 128 ... 512 training rows on the operand planes (fp16 pairs): the tile GEMM has 8 ... 32
  // tiles for 256 CUs there (22 us whatever the size); one 64-row block x 16 columns per workgroup instead, same planes,
  // same statistics partials.  (Under SyncBN only where the concatenated batch would come here too: "the shards compute
  // what one process computes on the concatenated batch, bit for bit" holds because both sides run the same kernel.)
  PlanesMid,
  // ... on fp32 operands (exact-fp32 MFMA) off the planes path (ragged rows, exact-fp32 / bf16x6 descriptors), 65 ... 512
  // rows, instead of the thin GEMM + its reduce or an 8 ... 32-tile GEMM
  F32Mid,
};
enum class Stats : uint8_t {   // BatchNorm statistics of a training forward
  None,
  InLayer,                     // small batches: Linear, statistics, finalize, apply in one small_layer.hip launch (tile bitmap)
  Small,                       // small batches: the Linear, then the rest in one launch (bn_small_fwd_kernel, row bitmap)
  // The statistics finalize inside the apply launch (bn_apply_kernel, BnApplyArgs::fin): local statistics, <= 4 groups (256
  // rows).  Measured same-box, step in ms with / without: B = 96 0.312 / 0.319, 128 0.295 / 0.300,
  // 256 0.298 / 0.304 -- and, when tried up to 16 groups, 512 0.353 / 0.351, 1,024 0.419 / 0.391: the dependent prologue in
  // every workgroup costs what the 4.9 us launch did as soon as there are more than a few groups (round 2 saw the same at 64).
  InApply,
  Finalize,                    // a finalize launch of its own
};
enum class Bwd : uint8_t {     // backward of a hidden layer's Linear in training (eval_bn: PlanesPair or F32Pair, or First)
  PlanesPair, F32Pair,         // dX = dz W and dW = dz^T a in one launch, on the operand planes / on fp32
  SmallLayer, SmallLayerDw,    // dX and the layer below's BatchNorm backward in one small_layer.hip launch; dW a GEMM / in it
  InAbove,                     // first layer: dW1 follows its BatchNorm backward in layer 1's launch (when in the range) ...
  First,                       // ... else on the family of its forward Linear: skinny.hip / gemm_tn_reduced
};
struct LayerRoute {
  Lin lin;
  Stats stats;                 // InLayer: the tile-format bitmap (pl_workspace_bitmap_format)
  Bwd bwd;
  int groups;                  // 64-row statistics groups the Linear's epilogue emits
  // BatchNorm-backward pass 1 of this layer is folded into the epilogue of the dX GEMM of layer l+1 (which produces its
  // incoming gradient) whenever that GEMM is a planes GEMM: every hidden layer but the top one.  The top layer's incoming
  // gradient comes from the 51-wide output layer (g = dy W5, skinny.hip): that kernel carries the same epilogue.
  bool bnr_fused;
};
// the fused train step's MSE: launch_small_mse on the slabs the last hidden layer's launch left (small_head); the output
// Linear's slab reduce folded into the MSE pass (one launch less, the same bits); y from the forward, then mse_partial_only
enum class Loss : uint8_t { SmallMse, FromSlabs, PartialOnly };

// Workspace plan; every region starts on a 256-byte boundary.
struct Ws {
  int L, G, RC;
  std::vector<size_t> z, act, bits, mean, rstd, dbpart;
  size_t stat, scale, shift, coef, ga, gb, dz, slabs, outpart, dyout, mse, total;
  size_t act_bytes, bits_bytes;
  size_t slab_floats;                 // size of the `slabs` region (also the thin GEMMs' split-K scratch)
  // PL_F16X3 planes path
  bool planes;
  int pkind;                          // PlaneOut::kind: 2 fp16 pair (PL_F16X3), 1 bf16 (PL_BF16)
  std::vector<size_t> actp, wp;       // activation planes of layers 0..L-2, weight planes of layers 1..L-1
  std::vector<size_t> sactp;          // small / ragged batches off the planes path, PL_F16X3: activation planes of layers 0..L-2
                                      // written by the layer kernels' tails (small_layer.hip: the fp16-planes contraction)
  std::vector<char> act_f32;          // is the fp32 activation of layer l materialised?
  size_t dzp, amax, dzscale;
  // partial sums whose combine is deferred to the ONE reduce launch at the end of a backward range
  size_t skp_out, skp_in;             // skinny weight-gradient partials of the output / input layer
  std::vector<size_t> wslab;          // split-K slabs of the 1024-wide weight gradients, one set per layer (planes path)
  // the route
  std::vector<LayerRoute> layer;
  bool bn_small;                      // the BatchNorm of every hidden layer in small-batch launches (Stats InLayer / Small)
  bool small_layer;                   // ... and layers 1.. in the small_layer.hip launches (Stats InLayer, Bwd SmallLayer*)
  bool top_fused;                     // the output layer and the top hidden layer's BatchNorm backward in one launch
  bool adam_rides;                    // the AdamW step of pl_lifter_train_step rides in the backward launches
  bool small_f16;                     // the small-batch layer launches contract on the fp16 planes in sactp
  bool eval_small;                    // pl_lifter_fwd_eval on the layer kernels of small_layer.hip
  bool out_narrow;                    // output Linear forward: launch_skinny_narrow_out (else the tile GEMM)
  bool out_skinny;                    // output Linear backward: skinny.hip (else gemm_tn_reduced, colsum, an NN GEMM)
  Loss loss;
};

Ws plan(const PLDesc* d, int64_t B) {
  Ws w;
  w.L = 1 + 2 * d->num_stage;
  const int H = d->hidden;
  w.G = gemm_stat_groups((int)B);
  w.RC = bwd_row_chunks((int)B, H);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o = (size_t)align_up((int64_t)(o + bytes), 256);
    return at;
  };
  w.act_bytes = (size_t)B * H * sizeof(float);
  // (at least H words: the tile-format bitmap of the small-batch layer kernels, small_layer.hip)
  w.bits_bytes = std::max((size_t)B * bitmap_words_per_row(H), (size_t)H) * sizeof(uint64_t);
  w.pkind = planes_kind(d, B);
  w.planes = w.pkind != 0;
  for (int l = 0; l < w.L; ++l) {
    // planes path: a layer's output is kept in fp32 only where something reads it as fp32 -- the skip connection
    // (even layers) and the output Linear (last layer); the odd layers feed GEMMs only and exist as planes
    const bool f32 = !w.planes || (l % 2 == 0) || l == w.L - 1;
    w.act_f32.push_back(f32 ? 1 : 0);
    w.z.push_back(take(w.act_bytes));
    w.act.push_back(f32 ? take(w.act_bytes) : 0);
    w.bits.push_back(take(w.bits_bytes));
    w.mean.push_back(take((size_t)H * 4));
    w.rstd.push_back(take((size_t)H * 4));
    w.dbpart.push_back(take((size_t)w.RC * H * 4));
  }
  const int Pmax = std::max(std::max(w.G, skinny_stat_groups((int)B)), w.RC);
  // per rank: two sets of at most Pmax partial rows, and (planes path under SyncBN) the {max|dy|, max|zhat|} pairs of
  // BatchNorm-backward pass 1 behind them
  const size_t amax_pairs = std::max((size_t)((H + 255) / 256) * w.RC, (size_t)(B / 64 + 1) * (H / 32 + 1));
  w.stat = take((size_t)sync_world(d) * ((size_t)2 * Pmax * H + 2 * amax_pairs) * 4);
  w.scale = take((size_t)w.L * H * 4);
  w.shift = take((size_t)w.L * H * 4);
  w.coef = take((size_t)3 * H * 4);
  w.ga = take(w.act_bytes);
  w.gb = take(w.act_bytes);
  w.dz = take(w.act_bytes);
  size_t slab = 0;
  auto need = [&](int M, int N) {
    const int s = tn_splits(M, N, (int)B);
    if (s > 1) slab = std::max(slab, (size_t)s * M * N * 4);
  };
  need(H, d->in_dim);
  need(H, H);
  need(d->out_dim, H);
  {
    const int so = out_splits((int)B, d->out_dim, H);
    if (so > 1) slab = std::max(slab, (size_t)so * B * d->out_dim * 4);
    // partials of the skinny-layer kernels (skinny.hip)
    slab = std::max(slab, (size_t)skinny_chunks((int)B) * std::max(d->in_dim, d->out_dim) * H * 4);
    slab = std::max(slab, skinny_narrow_out_part_floats((int)B, H) * 4);
    if (B <= kThinGemmMaxM && B % 128) slab = std::max(slab, thin_gemm_scratch_floats((int)B, H, H) * 4);
    if (B <= kThinGemmMaxM) slab = std::max(slab, (size_t)(H / 16 + 1) * B * 64 * 4);    // output-layer slabs of small_layer.hip
  }
  w.slab_floats = slab / 4;
  w.slabs = take(slab);
  w.outpart = take((size_t)std::max(colsum_chunks((int)B), skinny_in_chunks((int)B)) * d->out_dim * 4);
  w.dyout = take((size_t)B * d->out_dim * 4);                 // d loss / d y of the fused train step
  // (64 partials of launch_small_mse.  The loss partials moved to the end of the workspace when the skeleton terms' partials
  // joined them, below; these bytes stay reserved so that every other buffer keeps the address it had)
  const size_t mse_bytes = std::max(pl_mse_scratch_bytes(B * d->out_dim), (size_t)256);
  take(mse_bytes);
  w.dzp = w.amax = w.dzscale = 0;
  w.skp_out = take((size_t)skinny_in_chunks((int)B) * d->out_dim * H * 4);
  w.skp_in = take((size_t)skinny_in_chunks((int)B) * d->in_dim * H * 4);
  if (w.planes) {
    w.wslab.push_back(0);
    for (int l = 1; l < w.L; ++l) w.wslab.push_back(take((size_t)tn_splits(H, H, (int)B) * H * H * 4));
    for (int l = 0; l + 1 < w.L; ++l) w.actp.push_back(take(w.act_bytes));           // two fp16 planes = 4 B per element
    w.wp.push_back(0);
    for (int l = 1; l < w.L; ++l) w.wp.push_back(take((size_t)H * H * 4));
    w.dzp = take(w.act_bytes);
    w.amax = take(std::max((size_t)((H + 255) / 256) * w.RC, (size_t)(B / 64) * (H / 32)) * 2 * 4);
    w.dzscale = take((size_t)w.L * 2 * 4);
  }
  if (d->dtype == PL_F16X3 && B <= kThinGemmMaxM)
    for (int l = 0; l + 1 < w.L; ++l) w.sactp.push_back(take(w.act_bytes));           // two fp16 planes = 4 B per element
  // the loss pass's partial sums and, behind them, those of the skeleton terms (skeleton.hip): one run for the finalisers
  w.mse = take(mse_bytes + sk::kMaxGroups * sizeof(float));
  w.total = o;

  const int world = sync_world(d);
  const bool first_ok = small_first_ok(d->in_dim), mid_ok = B * world <= 512 && small_layer_ok(2, H, H);
  w.bn_small = d->bn && !w.planes && world == 1 && B >= 2 && B <= kBnSmallRows;
  w.small_layer = w.bn_small && small_layer_ok((int)B, H, H);
  w.top_fused = w.small_layer && small_top_ok(d->out_dim);
  const bool small_head = w.top_fused && (d->num_stage > 0 || first_ok);
  w.adam_rides = small_head && H % 128 == 0;
  // PL_F16X3 descriptors: the small-batch layer kernels contract on fp16 planes (three MFMAs per product) instead of exact
  // fp32 MFMAs -- forward and evaluation; the first layer's launch (which must then be one of them) writes the first planes.
  w.small_f16 = d->dtype == PL_F16X3 && !w.sactp.empty() && first_ok;
  w.eval_small = d->bn && B <= kThinGemmMaxM && small_layer_ok(2, H, H) && first_ok && small_top_ok(d->out_dim);
  w.out_narrow = skinny_narrow_out_supported(H, d->out_dim);
  w.out_skinny = skinny_supported(d->out_dim, H);
  const int so = w.out_narrow ? skinny_narrow_out_splits((int)B, H) : 0;
  w.loss = small_head ? Loss::SmallMse : (so && mse_from_slabs_supported(so, d->out_dim)) ? Loss::FromSlabs : Loss::PartialOnly;
  for (int l = 0; l < w.L; ++l) {
    LayerRoute r;
    if (l == 0) r.lin = skinny_supported(d->in_dim, H) ? Lin::Skinny : Lin::Gemm;
    else if (w.planes) r.lin = w.pkind == 2 && mid_ok ? Lin::PlanesMid : Lin::Planes;
    else r.lin = d->bn && d->dtype != PL_BF16 && B > kBnSmallRows && mid_ok ? Lin::F32Mid : Lin::Gemm;
    r.groups = r.lin == Lin::Skinny ? skinny_stat_groups((int)B) : w.G;
    const bool tile = w.small_layer && (l > 0 || first_ok);
    if (!d->bn) r.stats = Stats::None;
    else if (w.bn_small) r.stats = tile ? Stats::InLayer : Stats::Small;
    else r.stats = world == 1 && r.groups >= 1 && r.groups <= 4 ? Stats::InApply : Stats::Finalize;
    if (l == 0) r.bwd = tile && w.L > 1 ? Bwd::InAbove : Bwd::First;
    else if (!w.small_layer) r.bwd = w.planes ? Bwd::PlanesPair : Bwd::F32Pair;
    else r.bwd = H % 128 == 0 ? Bwd::SmallLayerDw : Bwd::SmallLayer;
    r.bnr_fused = w.planes && (l < w.L - 1 || w.out_skinny);      // (the planes path implies BatchNorm)
    w.layer.push_back(r);
  }
  return w;
}

// Where BatchNorm-backward pass 1 of one layer puts its output: this rank's slab of the gather buffer -- rc partial rows of
// sum dy, rc of sum dy zhat and, behind them, n_amax {max|dy|, max|zhat|} pairs (PL_F16X3: the range bound of dz).  One
// rank: the sums at the head of the buffer and the maxima in the workspace's own amax region, as before round 3.
struct BnrSlab {
  float *mine, *amax_mine, *amax0;     // this rank's partial sums / maxima; rank 0's maxima (what the finalize kernel walks)
  int64_t floats_per_rank;
  int world;
};
BnrSlab bnr_slab(const PLDesc* d, const Ws& w, void* ws, int rc, int n_amax, bool eval_bn) {
  BnrSlab b;
  float* stat = reinterpret_cast<float*>(static_cast<char*>(ws) + w.stat);
  b.world = eval_bn ? 1 : sync_world(d);
  const int64_t sums = (int64_t)2 * rc * d->hidden;
  if (b.world == 1) {
    b.mine = stat;
    b.amax_mine = b.amax0 = w.amax ? reinterpret_cast<float*>(static_cast<char*>(ws) + w.amax) : nullptr;
    b.floats_per_rank = sums;
    return b;
  }
  b.floats_per_rank = sums + 2 * (int64_t)n_amax;
  b.mine = stat + (size_t)sync_rank(d) * b.floats_per_rank;
  b.amax_mine = b.mine + sums;
  b.amax0 = stat + sums;
  return b;
}

struct Layer {
  const float *W, *b;
  BnParams bn;
  float *gW, *gb, *ggamma, *gbeta;
  int K;
};

Layer layer_of(const PLDesc* d, const ParamLayout& pl_, float* grads, int l) {
  Layer y;
  const int H = d->hidden;
  y.K = l == 0 ? d->in_dim : H;
  y.W = d->params + pl_.off[4 * l];
  y.b = d->params + pl_.off[4 * l + 1];
  y.bn.gamma = d->params + pl_.off[4 * l + 2];
  y.bn.beta = d->params + pl_.off[4 * l + 3];
  y.bn.eps = d->bn_eps;
  y.bn.momentum = d->bn_momentum;
  y.bn.running_mean = d->bn_running ? d->bn_running + (size_t)l * 2 * H : nullptr;
  y.bn.running_var = d->bn_running ? d->bn_running + (size_t)l * 2 * H + H : nullptr;
  y.bn.batches = d->bn_batches ? d->bn_batches + l : nullptr;
  y.gW = grads ? grads + pl_.off[4 * l] : nullptr;
  y.gb = grads ? grads + pl_.off[4 * l + 1] : nullptr;
  y.ggamma = grads ? grads + pl_.off[4 * l + 2] : nullptr;
  y.gbeta = grads ? grads + pl_.off[4 * l + 3] : nullptr;
  return y;
}

inline float* f32(void* ws, size_t off) { return reinterpret_cast<float*>(static_cast<char*>(ws) + off); }
inline uint64_t* u64(void* ws, size_t off) { return reinterpret_cast<uint64_t*>(static_cast<char*>(ws) + off); }

// what hidden layer l's forward saves in the workspace for its backward
inline BnSaved saved_of(const Ws& w, void* ws, int l) {
  return BnSaved{f32(ws, w.z[l]), u64(ws, w.bits[l]), f32(ws, w.mean[l]), f32(ws, w.rstd[l]), w.layer[l].stats == Stats::InLayer};
}

int check_ws(const Ws& w, void* ws, size_t bytes) {
  if (!ws) PL_FAIL(PL_EWORKSPACE, "workspace is NULL");
  if (reinterpret_cast<uintptr_t>(ws) & 255) PL_FAIL(PL_EWORKSPACE, "workspace not 256-byte aligned");
  if (bytes < w.total) PL_FAIL(PL_EWORKSPACE, "workspace too small: %zu < %zu bytes", bytes, w.total);
  return PL_OK;
}

inline unsigned short* u16(void* ws, size_t off) { return reinterpret_cast<unsigned short*>(static_cast<char*>(ws) + off); }
// the small-batch layer launches' fp16 input / output planes of hidden layer l (Ws::small_f16), or NULL
inline const unsigned short* sact_in(const Ws& w, void* ws, int l) { return w.small_f16 && l > 0 ? u16(ws, w.sactp[l - 1]) : nullptr; }
inline unsigned short* sact_out(const Ws& w, void* ws, int l) { return w.small_f16 && l + 1 < w.L ? u16(ws, w.sactp[l]) : nullptr; }

// operand planes of hidden layer l's weight: in the caller's persistent buffer (PLDesc.wplanes) or in the workspace
inline unsigned short* wplane(const PLDesc* d, const Ws& w, void* ws, int l) {
  if (d->wplanes) {
    const size_t per = (size_t)d->hidden * d->hidden * 2 * (w.pkind == 2 ? 2 : 1);
    return reinterpret_cast<unsigned short*>(static_cast<char*>(d->wplanes) + (size_t)(l - 1) * per);
  }
  return u16(ws, w.wp[l]);
}

// operand planes of every 1024-wide weight matrix (layers 1..L-1), from the fp32 parameter arena -- unless the
// caller keeps them current across calls (PLDesc.wplanes + wplanes_valid: pl_adamw_flat_planes refreshed them)
int split_weight_planes(const PLDesc* d, const ParamLayout& P, const Ws& w, void* ws, hipStream_t s) {
  if (d->wplanes && d->wplanes_valid) return PL_OK;
  if (d->wplanes && (reinterpret_cast<uintptr_t>(d->wplanes) & 15)) PL_FAIL(PL_EINVAL, "wplanes not 16-byte aligned");
  const int64_t n = (int64_t)d->hidden * d->hidden;
  for (int l = 1; l < w.L; ++l) {
    unsigned short* q = wplane(d, w, ws, l);
    PlaneOut po = {q, q + n, kWeightPlaneScale, nullptr, w.pkind};
    range_watch(po, PL_RANGE_SITE_LIFTER_WEIGHT);
    PL_TRY(launch_split_planes(d->params + P.off[4 * l], n, po, s));
  }
  return PL_OK;
}

PlanesGemmArgs planes_args(int pkind, const unsigned short* A, int64_t a_plane, int lda, const unsigned short* Bm,
                           int64_t b_plane, int ldb, float* C, int M, int N, int K, float out_scale,
                           const float* dyn_inv) {
  PlanesGemmArgs g = {};
  g.A = A; g.B = Bm; g.a_plane = a_plane; g.b_plane = b_plane; g.lda = lda; g.ldb = ldb;
  g.mode = pkind == 2 ? 2 : 0;                    // plp::kF16x3 / plp::kBf16
  g.out_scale = pkind == 2 ? out_scale : 1.0f;
  g.dyn_inv = pkind == 2 ? dyn_inv : nullptr;
  g.e.C = C; g.e.M = M; g.e.N = N; g.e.K = K; g.e.ldc = N; g.e.split_k = 1;
  return g;
}

int gemm_out_layer(bool narrow, const float* h, const float* W, const float* bias, float* y, int M, int N, int K,
                   float* slabs, hipStream_t s) {
  if (narrow) {
    SkinnyNarrowOutArgs a = {};
    a.h = h; a.W = W; a.B = M; a.H = K; a.N = N; a.part = slabs; a.reduce = true; a.bias = bias; a.y = y;
    return launch_skinny_narrow_out(a, s);
  }
  GemmArgs g = {};
  g.A = h; g.B = W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
  const int splits = out_splits(M, N, K);
  if (splits > 1) {
    g.C = slabs; g.split_k = splits;
    PL_TRY(launch_gemm_f32(kNT, g, s));
    return launch_reduce_slabs_bias(slabs, splits, M, N, bias, y, s);
  }
  g.C = y; g.bias = bias; g.split_k = 1;
  return launch_gemm_f32(kNT, g, s);
}

// C[M][N] (+slab reduce) = A^T B with A [K][M], B [K][N]
int gemm_tn_reduced(const float* A, int lda, const float* Bm, int ldb, float* C, int M, int N, int K,
                    float* slabs, hipStream_t s) {
  GemmArgs g = {};
  g.A = A; g.B = Bm; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = N;
  const int splits = tn_splits(M, N, K);
  if (splits > 1) {
    g.C = slabs; g.split_k = splits;
    PL_TRY(launch_gemm_f32(kTN, g, s));
    return launch_reduce_slabs(slabs, splits, (int64_t)M * N, C, s);
  }
  g.C = C; g.split_k = 1;
  return launch_gemm_f32(kTN, g, s);
}

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_version(void) { return PL_VERSION; }
extern "C" const char* pl_last_error(void) { return g_err; }

// the range guard's record (pl_internal.h range_record): per calling thread, like the error message
static thread_local uint32_t* g_range = nullptr;
uint32_t* pl::range_record() { return g_range; }
extern "C" int pl_range_monitor(void* record_or_null) {
  if (reinterpret_cast<uintptr_t>(record_or_null) & 3) PL_FAIL(PL_EINVAL, "pl_range_monitor: record not 4-byte aligned");
  g_range = static_cast<uint32_t*>(record_or_null);
  return PL_OK;
}

extern "C" int64_t pl_num_hidden(const PLDesc* d) { return d ? 1 + 2 * (int64_t)d->num_stage : PL_EINVAL; }
extern "C" int64_t pl_param_tensors(const PLDesc* d) { return d ? 4 * (1 + 2 * (int64_t)d->num_stage) + 2 : PL_EINVAL; }
extern "C" int64_t pl_param_offset(const PLDesc* d, int64_t i) {
  if (check_desc(d, false) != PL_OK) return PL_EINVAL;
  const ParamLayout p = param_layout(d);
  if (i < 0 || i >= (int64_t)p.off.size()) { set_error("tensor index %lld out of range", (long long)i); return PL_EINVAL; }
  return p.off[i];
}
extern "C" int64_t pl_param_numel(const PLDesc* d, int64_t i) {
  if (check_desc(d, false) != PL_OK) return PL_EINVAL;
  const ParamLayout p = param_layout(d);
  if (i < 0 || i >= (int64_t)p.numel.size()) { set_error("tensor index %lld out of range", (long long)i); return PL_EINVAL; }
  return p.numel[i];
}
extern "C" int64_t pl_param_arena_floats(const PLDesc* d) {
  if (check_desc(d, false) != PL_OK) return PL_EINVAL;
  return param_layout(d).total;
}

extern "C" size_t pl_wplanes_layer_bytes(const PLDesc* d) {
  if (check_desc(d, false) != PL_OK) return 0;
  if (!(d->bn && d->hidden % 128 == 0 && d->num_stage >= 1) || (d->dtype != PL_F16X3 && d->dtype != PL_BF16)) return 0;
  return (size_t)d->hidden * d->hidden * 2 * (d->dtype == PL_F16X3 ? 2 : 1);
}
extern "C" size_t pl_wplanes_bytes(const PLDesc* d) { return pl_wplanes_layer_bytes(d) * 2 * (size_t)(d ? d->num_stage : 0); }
extern "C" float pl_weight_plane_scale(void) { return kWeightPlaneScale; }

// refresh PLDesc.wplanes from the current parameters (what a forward call does first when wplanes_valid == 0)
extern "C" int pl_wplanes_refresh(const PLDesc* d, void* stream) {
  PL_TRY(check_desc(d, true));
  PLDesc t = *d;
  t.wplanes_valid = 0;
  const Ws w = plan(&t, 128);            // any batch on the planes path: only the layer count and plane kind are used
  if (!d->wplanes || !w.planes) PL_FAIL(PL_EINVAL, "pl_wplanes_refresh: this descriptor has no weight planes");
  return split_weight_planes(&t, param_layout(&t), w, nullptr, (hipStream_t)stream);
}

extern "C" size_t pl_workspace_bytes(const PLDesc* d, int64_t B) {
  if (check_desc(d, false) != PL_OK || B <= 0) return 0;
  return plan(d, B).total;
}

extern "C" int pl_workspace_view(const PLDesc* d, int64_t B, int which, int64_t layer, size_t* off,
                                 size_t* size) {
  PL_TRY(check_desc(d, false));
  if (B <= 0 || !off || !size) PL_FAIL(PL_EINVAL, "pl_workspace_view: bad arguments");
  const Ws w = plan(d, B);
  if (layer < 0 || layer >= w.L) PL_FAIL(PL_EINVAL, "pl_workspace_view: layer %lld out of range", (long long)layer);
  const size_t hb = (size_t)d->hidden * 4;
  switch (which) {
    case 0: *off = w.z[layer]; *size = w.act_bytes; break;
    case 1:
      if (!w.act_f32[layer])
        PL_FAIL(PL_EINVAL, "pl_workspace_view: the planes path keeps the output of hidden layer %lld as 16-bit planes only", (long long)layer);
      *off = w.act[layer]; *size = w.act_bytes; break;
    case 2: *off = w.bits[layer]; *size = w.bits_bytes; break;
    case 3: *off = w.mean[layer]; *size = hb; break;
    case 4: *off = w.rstd[layer]; *size = hb; break;
    default: PL_FAIL(PL_EINVAL, "pl_workspace_view: which=%d", which);
  }
  return PL_OK;
}

extern "C" int pl_workspace_bitmap_format(const PLDesc* d, int64_t B, int64_t layer) {
  PL_TRY(check_desc(d, false));
  if (B <= 0 || layer < 0 || layer >= 1 + 2 * (int64_t)d->num_stage) PL_FAIL(PL_EINVAL, "pl_workspace_bitmap_format: bad arguments");
  return plan(d, B).layer[layer].stats == Stats::InLayer ? 1 : 0;
}

// ---------------------------------------------------------------------------------------
// forward, eval mode
// ---------------------------------------------------------------------------------------
extern "C" int pl_lifter_fwd_eval(const PLDesc* d, const float* x, float* y, int64_t B, void* ws,
                                  size_t ws_bytes, void* stream) {
  PL_TRY(check_desc(d, true));
  if (!x || !y) PL_FAIL(PL_EINVAL, "pl_lifter_fwd_eval: null x/y");
  // (x meets element code -- small_first_fwd_kernel -- or launch_gemm_f32's own gate here: no alignment is asked of it)
  if (B <= 0) PL_FAIL(PL_ESHAPE, "pl_lifter_fwd_eval: B=%lld", (long long)B);
  const Ws w = plan(d, B);
  PL_TRY(check_ws(w, ws, ws_bytes));
  const ParamLayout P = param_layout(d);
  hipStream_t s = (hipStream_t)stream;
  const int H = d->hidden;
  // Small and ragged batches (everything the thin GEMMs took: M <= 512 rows off the tile grid): one launch per hidden layer
  // -- Linear, the BatchNorm fold on the running statistics, ReLU, residual -- on the layer kernels of small_layer.hip with
  // the grid also over 64-row blocks, the first layer on its vector-unit form, the output layer from the slabs the last
  // launch leaves: 6 launches instead of 16 at B = 64 (97 -> 47 us), every row the same bits whatever the batch.
  // (whole-tile batches up to 512 rows, too: on the operand-planes path an evaluation of 128 ... 512 rows is ~20 launches of
  //  8 ... 32 tiles each -- 143 us at any of these sizes -- where the layer kernels take 50 ... 110 us)
  if (w.eval_small) {
    const float* a_in = x;
    for (int l = 0; l < w.L; ++l) {
      const Layer ly = layer_of(d, P, nullptr, l);
      const float* resid = (l >= 2 && (l % 2) == 0) ? f32(ws, w.act[l - 2]) : nullptr;
      const bool last = l == w.L - 1;
      // (a whole-tile batch's plan keeps no fp32 activation for the odd layers: their output goes through the z buffer)
      float* out = w.act_f32[l] ? f32(ws, w.act[l]) : f32(ws, w.z[l]);
      SmallLayerFwdArgs a = {};
      a.a = a_in; a.W = ly.W; a.bias = ly.b; a.bn = ly.bn; a.resid = resid; a.act = out;
      a.B = (int)B; a.H = H; a.K = ly.K; a.layer = l; a.first = l == 0;
      if (last) { a.W2 = d->params + P.off[4 * w.L]; a.ypart = f32(ws, w.slabs); a.O = d->out_dim; }
      a.a_planes = sact_in(w, ws, l); a.out_planes = sact_out(w, ws, l);
      PL_TRY(launch_small_layer_eval(a, s));
      a_in = out;
    }
    SmallHeadArgs h = {};
    h.ypart = f32(ws, w.slabs); h.NS = H / 16; h.B = (int)B; h.O = d->out_dim; h.bias = d->params + P.off[4 * w.L + 1]; h.y = y;
    return launch_small_out(h, s);
  }
  for (int l = 0; l < w.L; ++l) {
    const Layer ly = layer_of(d, P, nullptr, l);
    PL_TRY(launch_bn_fold_eval(ly.b, d->bn ? &ly.bn : nullptr, H, f32(ws, w.scale) + (size_t)l * H,
                               f32(ws, w.shift) + (size_t)l * H, s));
  }
  const float* a_in = x;
  if (w.planes) PL_TRY(split_weight_planes(d, P, w, ws, s));
  const int64_t BH = B * H;
  for (int l = 0; l < w.L; ++l) {
    const Layer ly = layer_of(d, P, nullptr, l);
    // (planes path: the eval-mode output of an odd layer goes through its z buffer -- its fp32 activation is not kept)
    float* out = w.act_f32[l] ? f32(ws, w.act[l]) : f32(ws, w.z[l]);
    GemmArgs g = {};
    g.A = a_in; g.B = ly.W; g.C = out;
    g.M = (int)B; g.N = H; g.K = ly.K; g.lda = ly.K; g.ldb = ly.K; g.ldc = H; g.split_k = 1;
    g.arith = arith_of(d);
    g.col_scale = f32(ws, w.scale) + (size_t)l * H;
    g.col_shift = f32(ws, w.shift) + (size_t)l * H;
    g.relu = 1;
    if (l >= 2 && (l % 2) == 0) g.resid = f32(ws, w.act[l - 2]);
    g.thin_scratch = f32(ws, w.slabs); g.thin_scratch_floats = w.slab_floats;
    if (w.planes && l > 0) {
      PlanesGemmArgs pg = planes_args(w.pkind, u16(ws, w.actp[l - 1]), BH, H, wplane(d, w, ws, l), (int64_t)H * H, H, out, (int)B, H, H,
                                      1.0f / (kActPlaneScale * kWeightPlaneScale), nullptr);
      pg.e.col_scale = g.col_scale; pg.e.col_shift = g.col_shift; pg.e.relu = 1; pg.e.resid = g.resid;
      PL_TRY(launch_gemm_planes(kNT, pg, s));
    } else {
      PL_TRY(launch_gemm_f32(kNT, g, s));
    }
    if (w.planes && l + 1 < w.L) {
      PlaneOut po = {u16(ws, w.actp[l]), u16(ws, w.actp[l]) + BH, kActPlaneScale, nullptr, w.pkind};
      range_watch(po, range_site_act(l));
      PL_TRY(launch_split_planes(out, BH, po, s));
    }
    a_in = out;
  }
  return gemm_out_layer(w.out_narrow, a_in, d->params + P.off[4 * w.L], d->params + P.off[4 * w.L + 1], y, (int)B,
                        d->out_dim, H, f32(ws, w.slabs), s);
}

// ---------------------------------------------------------------------------------------
// forward, training mode
// ---------------------------------------------------------------------------------------
// eval_bn: the forward of model.eval() computed by the TRAINING kernels, so that everything a backward pass needs is
// saved in the workspace (pre-activations, ReLU bitmaps): BatchNorm normalises with the running statistics (which are
// not touched), Dropout is the identity.  pl_lifter_fwd_eval is the fast, nothing-saved form of the same function.
static int fwd_saved_impl(const PLDesc* d, const float* x, float* y, int64_t B, void* ws, size_t ws_bytes,
                          uint64_t seed, uint64_t step, const uint64_t* inject_keep, void* stream, bool eval_bn,
                          bool defer_out_reduce = false);

extern "C" int pl_lifter_fwd_train(const PLDesc* d, const float* x, float* y, int64_t B, void* ws,
                                   size_t ws_bytes, uint64_t seed, uint64_t step,
                                   const uint64_t* inject_keep, void* stream) {
  return fwd_saved_impl(d, x, y, B, ws, ws_bytes, seed, step, inject_keep, stream, false);
}

extern "C" int pl_lifter_fwd_eval_saved(const PLDesc* d, const float* x, float* y, int64_t B, void* ws,
                                        size_t ws_bytes, void* stream) {
  return fwd_saved_impl(d, x, y, B, ws, ws_bytes, 0, 0, nullptr, stream, true);
}

static int fwd_saved_impl(const PLDesc* d, const float* x, float* y, int64_t B, void* ws, size_t ws_bytes,
                          uint64_t seed, uint64_t step, const uint64_t* inject_keep, void* stream, bool eval_bn,
                          bool defer_out_reduce) {
  PL_TRY(check_desc(d, true));
  if (!x || !y) PL_FAIL(PL_EINVAL, "pl_lifter_fwd_train: null x/y");
  // x: the first Linear on skinny.hip stages whole 64-row groups of it as float4 (skinny_wide_out_kernel).  y is written by
  // element kernels or behind launch_gemm_f32's own gate.
  PL_REQUIRE_ALIGNED16("pl_lifter_fwd_train", x);
  if (B <= 0) PL_FAIL(PL_ESHAPE, "pl_lifter_fwd_train: B=%lld", (long long)B);
  if (d->bn && B < 2 && !eval_bn)
    PL_FAIL(PL_EBATCH, "Expected more than 1 value per channel when training (B=%lld)", (long long)B);
  const Ws w = plan(d, B);
  PL_TRY(check_ws(w, ws, ws_bytes));
  const ParamLayout P = param_layout(d);
  hipStream_t s = (hipStream_t)stream;
  const int H = d->hidden;
  const size_t inj_stride = (size_t)B * bitmap_words_per_row(H);
  const float* a_in = x;
  const int64_t BH = B * H;
  if (w.planes) PL_TRY(split_weight_planes(d, P, w, ws, s));
  // (small batches, fused train step: the last hidden layer's launch leaves the output Linear's slabs -- small_layer.hip)
  const bool head_slabs = defer_out_reduce && w.loss == Loss::SmallMse;
  for (int l = 0; l < w.L; ++l) {
    const Layer ly = layer_of(d, P, nullptr, l);
    const LayerRoute& r = w.layer[l];
    const Stats st = eval_bn ? Stats::None : r.stats;         // (eval_bn: the running statistics, below)
    GemmArgs g = {};
    g.A = a_in; g.B = ly.W; g.C = f32(ws, w.z[l]); g.bias = ly.b;
    g.M = (int)B; g.N = H; g.K = ly.K; g.lda = ly.K; g.ldb = ly.K; g.ldc = H; g.split_k = 1;
    g.arith = arith_of(d);
    g.thin_scratch = f32(ws, w.slabs); g.thin_scratch_floats = w.slab_floats;
    float* stat = f32(ws, w.stat);
    const float* resid = (l >= 2 && (l % 2) == 0) ? f32(ws, w.act[l - 2]) : nullptr;
    const BnSaved sv = saved_of(w, ws, l);
    const DropKey drop = dropout_key(eval_bn ? 0.f : d->p_dropout, seed, step, l,
                                     inject_keep ? inject_keep + (size_t)l * inj_stride : nullptr, eval_bn ? nullptr : d->step_dev);
    if (st == Stats::InLayer) {
      SmallLayerFwdArgs a = {};
      a.a = a_in; a.W = ly.W; a.bias = ly.b; a.bn = ly.bn; a.saved = sv; a.resid = resid; a.act = f32(ws, w.act[l]);
      a.B = (int)B; a.H = H; a.K = ly.K; a.layer = l; a.drop = drop; a.first = l == 0;
      if (head_slabs && l == w.L - 1) { a.W2 = d->params + P.off[4 * w.L]; a.ypart = f32(ws, w.slabs); a.O = d->out_dim; }
      a.a_planes = sact_in(w, ws, l); a.out_planes = sact_out(w, ws, l);
      PL_TRY(launch_small_layer_fwd(a, s));
      a_in = a.act;
      continue;
    }
    if (st == Stats::InApply || st == Stats::Finalize) {
      g.stat_sum = stat + (size_t)sync_rank(d) * 2 * r.groups * H;
      g.stat_m2 = g.stat_sum + (size_t)r.groups * H;
    }
    if (r.lin == Lin::Skinny) {
      SkinnyWideOutArgs a = {};
      a.X = a_in; a.W = ly.W; a.bias = ly.b; a.out = g.C; a.B = (int)B; a.K = ly.K; a.H = H;
      a.stat_sum = g.stat_sum; a.stat_m2 = g.stat_m2;
      PL_TRY(launch_skinny_wide_out(a, s));
    } else if (r.lin == Lin::PlanesMid || r.lin == Lin::F32Mid) {
      SmallLinearStatsArgs q = {};
      if (r.lin == Lin::PlanesMid) q.a_planes = u16(ws, w.actp[l - 1]); else q.a = a_in;
      q.W = ly.W; q.bias = ly.b; q.z = sv.z; q.M = (int)B; q.H = H; q.K = H;
      q.stat_sum = g.stat_sum; q.stat_m2 = g.stat_m2; q.groups = r.groups;
      PL_TRY(launch_small_linear_stats(q, s));
    } else if (r.lin == Lin::Planes) {
      PlanesGemmArgs pg = planes_args(w.pkind, u16(ws, w.actp[l - 1]), BH, H, wplane(d, w, ws, l), (int64_t)H * H, H, g.C, (int)B, H, H,
                                      1.0f / (kActPlaneScale * kWeightPlaneScale), nullptr);
      pg.e.bias = ly.b; pg.e.stat_sum = g.stat_sum; pg.e.stat_m2 = g.stat_m2;
      PL_TRY(launch_gemm_planes(kNT, pg, s));
    } else {
      PL_TRY(launch_gemm_f32(kNT, g, s));
    }
    BnApplyArgs ap = {};
    BnFinalizeArgs fin = {};
    fin.G = r.groups; fin.group_rows = 64; fin.world = sync_world(d); fin.B = (int)B; fin.H = H;
    fin.bn = ly.bn; fin.mean = sv.mean; fin.rstd = sv.rstd;
    fin.scale = f32(ws, w.scale) + (size_t)l * H; fin.shift = f32(ws, w.shift) + (size_t)l * H;
    if (d->bn && eval_bn) {
      PL_TRY(launch_bn_eval_stats(fin, s));
      ap.scale = fin.scale; ap.shift = fin.shift;
    } else if (st == Stats::InApply) {
      fin.stat = stat;
      ap.fin = fin;
    } else if (st == Stats::Finalize) {
      PL_TRY(sync_gather(d, stat, (int64_t)2 * r.groups * H, s));
      fin.stat = stat;
      PL_TRY(launch_bn_finalize(fin, s));
      ap.scale = fin.scale; ap.shift = fin.shift;
    } else if (st == Stats::Small) {
      BnSmallFwdArgs a = {};
      a.saved = sv; a.bn = ly.bn; a.resid = resid; a.act = f32(ws, w.act[l]); a.B = (int)B; a.H = H; a.drop = drop;
      PL_TRY(launch_bn_small_fwd(a, s));
      a_in = a.act;
      continue;
    }
    ap.z = sv.z; ap.resid = resid; ap.act = w.act_f32[l] ? f32(ws, w.act[l]) : nullptr; ap.bits = sv.bits;
    ap.B = (int)B; ap.H = H; ap.drop = drop;
    ap.planes.scale = kActPlaneScale;
    if (w.planes && l + 1 < w.L) {
      ap.planes.h = u16(ws, w.actp[l]); ap.planes.l = ap.planes.h + BH; ap.planes.kind = w.pkind;
      range_watch(ap.planes, range_site_act(l));
    }
    PL_TRY(launch_bn_apply(ap, s));
    a_in = ap.act;
  }
  if (head_slabs) return PL_OK;
  if (defer_out_reduce) {   // (the fused train step: y = bias + slabs is formed by the MSE pass, mse_partial_from_slabs)
    SkinnyNarrowOutArgs a = {};
    a.h = a_in; a.W = d->params + P.off[4 * w.L]; a.B = (int)B; a.H = H; a.N = d->out_dim; a.part = f32(ws, w.slabs);
    return launch_skinny_narrow_out(a, s);
  }
  return gemm_out_layer(w.out_narrow, a_in, d->params + P.off[4 * w.L], d->params + P.off[4 * w.L + 1], y, (int)B,
                        d->out_dim, H, f32(ws, w.slabs), s);
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
namespace pl {
namespace {

// What the parts of one backward range share.
struct BwdCtx {
  const PLDesc* d;
  const Ws& w;
  const ParamLayout& P;
  void* ws;
  hipStream_t s;
  const float *x, *dy;
  float *dx, *grads;
  int B, H, O;
  int l_hi, l_lo;
  float kscale;                 // 1 / (1 - p) of the dropout the forward applied
  bool eval_bn;
  bool small, sl;               // small batches: every BatchNorm in one launch; layers 1.. on the layer kernels (small_layer.hip)
  bool top_fused;               // the output layer and the top hidden layer's BatchNorm backward in one launch (dz of that layer: DZ)
  float* loss_out;              // the fused train step: the loss is finalised by a launch of this range
  int n_loss_part;              //   ... from this many partial sums in w.mse
  float loss_inv_n;             //   ... times this (1 / (B O); the mpjpe criterion: 1 / (B J))
  // the AdamW step carried by the backward launches (pl_lifter_train_step) or run behind them
  const PLAdamWStep* adam;
  bool adam_rides;
  // bias gradients and split-K slabs = column sums of partials; all of them are reduced by ONE launch at the end
  std::vector<RowJob> jobs;
  // ... but for the slab sum of the layer above where the next pair launch carries it (slab_sum_rides_below): R > 0
  RowJob pending = {};

  float* buf(size_t off) const { return f32(ws, off); }
  float* GA() const { return buf(w.ga); }
  float* GB() const { return buf(w.gb); }
  float* DZ() const { return buf(w.dz); }
  int64_t BH() const { return (int64_t)B * H; }
  // gradient w.r.t. layer l's activation: GA for layer 0 and even layers, GB for odd ones
  const float* gin(int l) const { return (l % 2 == 1) ? GB() : GA(); }
  // where dz of layer l lives (layer kernels: alternating -- a launch reads dz_l and writes dz_{l-1})
  float* dzbuf(int l) const { return (sl && (l & 1)) ? GB() : DZ(); }
  bool planes_pair(int l) const { return w.layer[l].bwd == Bwd::PlanesPair; }      // layer l's dz feeds the planes GEMM pair
  // fp16 planes of dz are range-scaled: {S, 1/S} of layer l on the device, or NULL
  float* dzs(int l) const { return (planes_pair(l) && w.pkind == 2) ? buf(w.dzscale) + 2 * l : nullptr; }
  void job(const float* part, float* out, int R, int Hj, int kind, int transK) { jobs.push_back(RowJob{part, out, R, Hj, kind, transK}); }
  // small batches (small_layer.hip): what describes a layer's BatchNorm -- and its bitmap's format
  SmallBnLayer bn_layer(int l) const {
    const Layer y = layer_of(d, P, grads, l);
    return SmallBnLayer{saved_of(w, ws, l), y.bn.gamma, y.ggamma, y.gbeta, y.gb};
  }
  // which slice of the arena rides with a launch
  AdamWRide ride(int64_t lo, int64_t hi) const {
    AdamWRide r = {};
    r.p = const_cast<float*>(d->params) + lo; r.g = grads + lo; r.m = adam->m + lo; r.v = adam->v + lo; r.n = hi - lo;
    r.lr = adam->lr; r.beta1 = adam->beta1; r.beta2 = adam->beta2; r.eps = adam->eps; r.wd = adam->weight_decay; r.gscale = 1.0f;
    r.t = adam->t; r.lr_dev = adam->lr_dev; r.t_dev = adam->t_dev;
    return r;
  }
  // ... and that slice of the averaged weights (adam->ema set)
  PLEma ema_at(int64_t lo) const {
    PLEma e = *adam->ema;
    e.e += lo;
    return e;
  }
};

// BatchNorm-backward pass 1 of layer l inside the epilogue of the GEMM that produces its incoming gradient
// (LayerRoute::bnr_fused): partial sums per 64-row block, and -- where the layer's dz leaves as fp16 planes (PL_F16X3, not the
// first layer) -- the range maxima per (64-row block, 64-column strip); the top layer's gradient comes from the skinny
// kernel, whose strips are 32 columns wide.
int bnr_amax_pairs(const BwdCtx& c, int l) { return (c.B / 64) * (c.H / (l == c.w.L - 1 ? 32 : 64)); }
BnrEpilogue bnr_of(const BwdCtx& c, int l) {
  const BnSaved sv = saved_of(c.w, c.ws, l);
  const bool scaled = c.w.pkind == 2 && l > 0;
  const BnrSlab slab = bnr_slab(c.d, c.w, c.ws, c.B / 64, scaled ? bnr_amax_pairs(c, l) : 0, c.eval_bn);
  BnrEpilogue b = {};
  b.z = sv.z; b.bits = sv.bits; b.mean = sv.mean; b.rstd = sv.rstd; b.kscale = c.kscale;
  b.part_dy = slab.mine; b.part_dyz = slab.mine + (size_t)(c.B / 64) * c.H;
  b.amax = scaled ? slab.amax_mine : nullptr;
  return b;
}
void set_bnr(GemmArgs& e, const BnrEpilogue& b) {     // the planes GEMM carries it in its epilogue fields
  e.bnr_z = b.z; e.bnr_bits = b.bits; e.bnr_mean = b.mean; e.bnr_rstd = b.rstd; e.bnr_kscale = b.kscale;
  e.bnr_part_dy = b.part_dy; e.bnr_part_dyz = b.part_dyz; e.bnr_amax = b.amax;
}

// The backward pair of a hidden layer on the planes, as its route decisions read it: shapes, mode, split and the two outputs
// (every such layer's pair has the same shapes).  The operands and what rides in dX's epilogue are the caller's to add.
void pair_problems(const Ws& w, int H, int B, float* g_out, float* dw_out, PlanesGemmArgs& nn, PlanesGemmArgs& tn) {
  const int64_t BH = (int64_t)B * H;
  nn = planes_args(w.pkind, nullptr, BH, H, nullptr, (int64_t)H * H, H, g_out, B, H, H, 1.0f / kWeightPlaneScale, nullptr);
  tn = planes_args(w.pkind, nullptr, BH, H, nullptr, BH, H, dw_out, H, H, B, 1.0f / kActPlaneScale, nullptr);
  tn.e.split_k = tn_splits(H, H, B);
}
// Is the split-K sum of layer l's weight gradient carried by the chained launch of layer l - 1's pair (gemm_planes16.h SLAB
// RIDE) rather than by the range's reduce launch?  Both layers run the planes pair in this call's range [.., l_lo], layer l
// leaves slabs, and the GEMM says its launch can take them (planes_pair_carries_slab_sum: the route, the slab count, the
// deal over the loader waves and dX's step count).
bool slab_sum_rides_below(const Ws& w, int H, int B, int l, int l_lo) {
  if (l - 1 < l_lo || l - 1 < 1 || l >= w.L) return false;
  if (w.layer[l].bwd != Bwd::PlanesPair || w.layer[l - 1].bwd != Bwd::PlanesPair) return false;
  const int splits = tn_splits(H, H, B);
  if (splits <= 1) return false;
  static float placeholder[4];                     // outputs that exist, for the route's sake; nothing is launched from here
  PlanesGemmArgs nn, tn;
  pair_problems(w, H, B, placeholder, placeholder, nn, tn);
  return planes_pair_carries_slab_sum(nn, tn, splits, (int64_t)H * H);
}

// The output layer (LinearModel.w2): dW = dy^T h, db = sum dy, g = dy W -> GA.  Three routes.
int bwd_output(BwdCtx& c) {
  const Ws& w = c.w;
  const int Bi = c.B, H = c.H, O = c.O;
  const float* W2 = c.d->params + c.P.off[4 * w.L];
  float* gW2 = c.grads + c.P.off[4 * w.L];
  float* gb2 = c.grads + c.P.off[4 * w.L + 1];
  const float* h = c.buf(w.act[w.L - 1]);
  if (c.top_fused) {
    SmallTopBwdArgs a = {};
    a.dy = c.dy; a.W2 = W2; a.h = h; a.B = Bi; a.H = H; a.O = O; a.gout = c.GA(); a.dW2 = gW2; a.db2 = gb2;
    a.top = c.bn_layer(w.L - 1); a.kscale = c.kscale; a.dz_top = c.DZ();
    a.mpart = c.buf(w.mse); a.np = c.n_loss_part; a.inv_n = c.loss_inv_n; a.loss = c.loss_out;
    a.tick = const_cast<uint64_t*>(c.d->step_dev);
    return launch_small_top_bwd(a, c.s);
  }
  if (w.out_skinny) {
    // dW5 partials, and -- the kernel holds every row of dy in its A fragments -- the bias gradient's partial column sums
    // (Round 3 tried this launch on a side stream -- nothing reads its output before the closing reduce, and it and the head of
    //  the chain below are both latency-bound -- forked and joined with events: 0.627 -> 0.660 ms per step eager, 0.644 -> 0.663
    //  replayed from a graph, same box: the two cross-stream dependencies cost more than the 13 us launch they hide.)
    SkinnyWideInArgs wi = {};
    wi.X = c.dy; wi.D = h; wi.B = Bi; wi.K = O; wi.H = H; wi.part = c.buf(w.skp_out); wi.xsum = c.buf(w.outpart);
    PL_TRY(launch_skinny_wide_in(wi, c.s));
    c.job(c.buf(w.skp_out), gW2, skinny_in_chunks(Bi), O * H, 0, 0);
    c.job(c.buf(w.outpart), gb2, skinny_in_chunks(Bi), O, 0, 0);
    SkinnyWideOutArgs wo = {};
    wo.X = c.dy; wo.W = W2; wo.out = c.GA(); wo.B = Bi; wo.K = O; wo.H = H; wo.w_transposed = true;
    if (!c.eval_bn && w.layer[w.L - 1].bnr_fused) wo.bnr = bnr_of(c, w.L - 1);   // pass 1 of the top hidden layer, on the block just produced
    return launch_skinny_wide_out(wo, c.s);
  }
  PL_TRY(gemm_tn_reduced(c.dy, O, h, H, gW2, O, H, Bi, c.buf(w.slabs), c.s));
  PL_TRY(launch_colsum_partial(c.dy, Bi, O, c.buf(w.outpart), c.s));
  c.job(c.buf(w.outpart), gb2, colsum_chunks(Bi), O, 0, 0);
  GemmArgs g = {};
  g.A = c.dy; g.B = W2; g.C = c.GA(); g.M = Bi; g.N = H; g.K = O; g.lda = O; g.ldb = H; g.ldc = H;
  g.split_k = 1;
  return launch_gemm_f32(kNN, g, c.s);
}

// Hidden layer l: from the gradient of its activation (gin) to dz, dgamma, dbeta and the bias gradient.  Four routes.
int bwd_layer_bn(BwdCtx& c, int l) {
  // small batches, layer kernels (small_layer.hip): the dX launch of layer l + 1 (launch_small_layer_bwd) or launch_small_top_bwd
  // already ran this layer's BatchNorm backward (dz_l sits in dzbuf(l)) unless this layer heads the range
  if (c.sl && (l < c.l_hi || c.top_fused)) return PL_OK;
  const Ws& w = c.w;
  const PLDesc* d = c.d;
  const int Bi = c.B, H = c.H;
  if (c.small) {
    // pass 1, the coefficients, dz, the bias gradient and dgamma / dbeta of this layer in one launch (small batches)
    BnSmallBwdArgs a = {};
    a.g = c.gin(l); a.layer = c.bn_layer(l); a.keep_scale = c.kscale; a.B = Bi; a.H = H; a.dz = c.dzbuf(l);
    return launch_bn_small_bwd(a, c.s);
  }
  const Layer ly = layer_of(d, c.P, c.grads, l);
  const LayerRoute& r = w.layer[l];
  const BnSaved sv = saved_of(w, c.ws, l);
  float* dzs = c.dzs(l);
  if (d->bn) {
    // pass 1 (column sums of dy and dy*zhat): a streaming kernel of its own, or -- round 2 -- already done by the
    // LDS-staged epilogue of the planes GEMM that produced `gin` (round 1 tried it in the dword-per-lane epilogue of
    // the fp32-operand GEMM: +17 us per GEMM for the 7.5 us kernel it removed)
    const bool fr = !c.eval_bn && r.bnr_fused;
    const int rc_l = fr ? Bi / 64 : w.RC;
    const int n_amax_l = fr ? bnr_amax_pairs(c, l) : ((H + 255) / 256) * w.RC;
    const BnrSlab slab = bnr_slab(d, w, c.ws, rc_l, dzs ? n_amax_l : 0, c.eval_bn);
    float* stat = c.buf(w.stat);
    if (!fr) {
      BnBwdReduceArgs a = {};
      a.g = c.gin(l); a.saved = sv; a.keep_scale = c.kscale; a.B = Bi; a.H = H; a.rc = rc_l;
      a.part_dy = slab.mine; a.part_dyz = slab.mine + (size_t)rc_l * H; a.part_amax = dzs ? slab.amax_mine : nullptr;
      PL_TRY(launch_bn_bwd_reduce(a, c.s));
    }
    // (fused: the partials were written by the GEMM / skinny epilogue that produced `gin`, into this rank's slab)
    if (!c.eval_bn) PL_TRY(sync_gather(d, stat, slab.floats_per_rank, c.s));
    BnBwdFinalizeArgs f = {};
    f.part = stat; f.RC = rc_l; f.world = c.eval_bn ? 1 : sync_world(d); f.rank = c.eval_bn ? 0 : sync_rank(d); f.B = Bi; f.H = H;
    f.gamma = ly.bn.gamma; f.rstd = sv.rstd; f.coef = c.buf(w.coef); f.dgamma = ly.ggamma; f.dbeta = ly.gbeta;
    f.part_amax = dzs ? slab.amax0 : nullptr; f.n_amax = n_amax_l; f.dz_scale = dzs; f.eval_mode = c.eval_bn ? 1 : 0;
    f.rstride = slab.floats_per_rank; f.amax_world = slab.world;
    PL_TRY(launch_bn_bwd_finalize(f, c.s));
  } else {
    PL_TRY(launch_fill(ly.ggamma, H, 0.f, c.s));
    PL_TRY(launch_fill(ly.gbeta, H, 0.f, c.s));
  }
  BnBwdDzArgs a = {};
  a.g = c.gin(l); a.saved = sv; a.coef = c.buf(w.coef); a.keep_scale = c.kscale; a.bn = d->bn; a.B = Bi; a.H = H; a.rc = w.RC;
  a.dz = c.planes_pair(l) ? nullptr : c.DZ(); a.part_db = c.buf(w.dbpart[l]);
  a.planes.scale = 1.0f; a.planes.dyn = dzs;
  if (c.planes_pair(l)) { a.planes.h = u16(c.ws, w.dzp); a.planes.l = a.planes.h + c.BH(); a.planes.kind = w.pkind; }
  PL_TRY(launch_bn_bwd_dz(a, c.s));
  c.job(c.buf(w.dbpart[l]), ly.gb, w.RC, H, 0, 0);
  return PL_OK;
}

// Hidden layer l: from dz to the gradient of the activation below (GA / GB; dx for layer 0) and the weight gradient.
// Six routes.
int bwd_layer_linear(BwdCtx& c, int l) {
  const Ws& w = c.w;
  const PLDesc* d = c.d;
  const int Bi = c.B, H = c.H;
  hipStream_t s = c.s;
  const Layer ly = layer_of(d, c.P, c.grads, l);
  const LayerRoute& r = w.layer[l];
  float* const GA = c.GA();
  float* const GB = c.GB();
  float* const DZ = c.DZ();
  float* const DZl = c.dzbuf(l);
  float* slabs = c.buf(w.slabs);
  const float* a_in = l == 0 ? c.x : (w.planes ? nullptr : c.buf(w.act[l - 1]));
  if (c.planes_pair(l)) {
    // dX = dz W (NN) and dW = dz^T a (TN, split-K slabs) on the planes: one launch
    float* dzs = c.dzs(l);
    const int splits = tn_splits(H, H, Bi);
    // this layer's own slabs: combined by the launch of the pair below where that carries the sum, else by the range's one
    // reduce launch; nothing reads them or gW in between
    float* wsl = c.buf(w.wslab[l]);
    PlanesGemmArgs nn, tn;
    pair_problems(w, H, Bi, (l % 2 == 1) ? GA : GB, splits > 1 ? wsl : ly.gW, nn, tn);
    nn.A = tn.A = u16(c.ws, w.dzp);
    nn.B = wplane(d, w, c.ws, l);
    tn.B = u16(c.ws, w.actp[l - 1]);
    if (w.pkind == 2) nn.dyn_inv = tn.dyn_inv = dzs ? dzs + 1 : nullptr;
    if (l % 2 == 1) nn.e.addend = GA;
    if (!c.eval_bn && w.layer[l - 1].bnr_fused) set_bnr(nn.e, bnr_of(c, l - 1));      // pass 1 of the layer below, on the block just produced
    const SlabSum above = {c.pending.part, c.pending.out, c.pending.R, (int64_t)c.pending.H};
    PL_TRY(launch_gemm_planes_pair(nn, tn, c.pending.R > 0 ? &above : nullptr, s));
    c.pending = RowJob{};
    if (splits > 1) {
      const RowJob sum = {wsl, ly.gW, splits, H * H, 1, 0};
      if (slab_sum_rides_below(w, H, Bi, l, c.l_lo)) c.pending = sum; else c.jobs.push_back(sum);
    }
  } else if (l > 0) {
    // off the planes path: dX = dz W (+ the skip gradient a residual block's first Linear receives in GA, added in the
    // epilogue) and dW = dz^T a_in
    GemmArgs g = {};
    g.A = DZl; g.B = ly.W; g.M = Bi; g.N = H; g.K = H; g.lda = H; g.ldb = H; g.ldc = H; g.split_k = 1;
    if (l % 2 == 1) { g.C = GA; g.addend = GA; } else { g.C = GB; }
    g.arith = arith_of(d);
    g.thin_scratch = slabs; g.thin_scratch_floats = w.slab_floats;   // (the pair runs as two launches off the tile grid)
    GemmArgs t = {};
    t.arith = g.arith;
    t.A = DZl; t.B = a_in; t.M = H; t.N = H; t.K = Bi; t.lda = H; t.ldb = H; t.ldc = H; t.split_k = 1; t.C = ly.gW;
    if (c.sl && (r.bwd == Bwd::SmallLayer || r.bwd == Bwd::SmallLayerDw)) {
      // small batches: dX and the BatchNorm backward of the layer below in one launch when that layer belongs to this
      // range; the weight gradient is one whole-K launch (K = B <= 64) or extra workgroups of the same launch
      const bool dw_rides = r.bwd == Bwd::SmallLayerDw;
      if (l - 1 < c.l_lo) {
        PL_TRY(launch_gemm_f32(kNN, g, s));
        return launch_gemm_f32(kTN, t, s);
      }
      const bool w1 = l == 1 && w.layer[0].bwd == Bwd::InAbove;
      // AdamW on this launch's spare workgroups: this layer's bias and BatchNorm parameters (their gradients came with the
      // launch before) and everything above them up to where the launch before started -- the weight matrix of layer
      // l + 1 (its gradient, too), or the output layer behind the top hidden layer
      AdamWRide ar = {};
      PLEma er = {};
      if (c.adam_rides) ar = c.ride(c.P.off[4 * l + 1], l == w.L - 1 ? c.P.total : c.P.off[4 * (l + 1) + 1]);
      if (c.adam_rides && c.adam->ema) er = c.ema_at(c.P.off[4 * l + 1]);
      SmallLayerBwdArgs a = {};
      a.dz = DZl; a.W = ly.W; a.B = Bi; a.H = H; a.K = H;
      if (l % 2 == 1) { a.addend = GA; a.gout = GA; }
      a.below = c.bn_layer(l - 1); a.kscale = c.kscale; a.dz_lo = c.dzbuf(l - 1);
      if (dw_rides) { a.a_in = a_in; a.dW = ly.gW; }
      if (w1) { a.x1 = c.x; a.dW1 = c.grads + c.P.off[0]; }
      a.K1 = d->in_dim;
      if (c.adam_rides) a.adam = &ar;
      if (c.adam_rides && c.adam->ema) a.ema = &er;
      PL_TRY(launch_small_layer_bwd(a, s));
      return dw_rides ? PL_OK : launch_gemm_f32(kTN, t, s);
    }
    // dX and dW share dz and are independent: ONE launch.
    // (Tried: dW on a side stream so that the next layer's BatchNorm-backward kernels overlap it --
    //  -2 % per step only: two single-GEMM workgroups do not fit one CU together, so dX and dW
    //  time-slice the CUs and the dual launch's co-residency is lost.  Same-box A/B, tools/ab_env.py.)
    const int splits = tn_splits(H, H, Bi);
    t.split_k = splits; t.C = splits > 1 ? slabs : ly.gW;
    PL_TRY(launch_gemm_f32_pair(g, t, s));
    if (splits > 1) PL_TRY(launch_reduce_slabs(slabs, splits, (int64_t)H * H, ly.gW, s));
  } else if (r.bwd == Bwd::InAbove && c.sl && c.l_hi > 0) {
    // (layer 0's weight gradient came with its BatchNorm backward, small_layer.hip)
  } else if (r.lin == Lin::Skinny) {
    SkinnyWideInArgs wi = {};
    wi.X = a_in; wi.D = DZ; wi.B = Bi; wi.K = ly.K; wi.H = H; wi.part = c.buf(w.skp_in);
    PL_TRY(launch_skinny_wide_in(wi, s));
    c.job(c.buf(w.skp_in), ly.gW, skinny_in_chunks(Bi), ly.K * H, 0, ly.K);
  } else {
    PL_TRY(gemm_tn_reduced(DZ, H, a_in, ly.K, ly.gW, H, ly.K, Bi, slabs, s));
  }
  if (l == 0 && c.dx) {
    GemmArgs g = {};
    g.A = DZ; g.B = ly.W; g.C = c.dx; g.M = Bi; g.N = d->in_dim; g.K = H; g.lda = H; g.ldb = d->in_dim;
    g.ldc = d->in_dim; g.split_k = 1;
    PL_TRY(launch_gemm_f32(kNN, g, s));
  }
  return PL_OK;
}

}  // namespace
}  // namespace pl

// Backward over the output layer (if do_output) and hidden layers l_hi .. l_lo (descending).
// The gradient flowing between two calls lives in the workspace (GA/GB), so the pass can be cut
// at any layer boundary: the data-parallel driver all-reduces the first half's gradients while
// the second half is still computing.
// loss_out != NULL (the fused train step): the MSE loss is finalised by this range's one reduce launch (a kind-2 job:
// mse_final_kernel's sum) and the device step counter ticks there, instead of in a launch of their own after the forward.
static int bwd_impl(const PLDesc* d, const float* x, const float* dy, int64_t B, void* ws, size_t ws_bytes,
                    float* dx, float* grads, void* stream, bool do_output, int l_hi, int l_lo, bool eval_bn = false,
                    float* loss_out = nullptr, int n_loss_part = 0, float loss_inv_n = 0.f, const PLAdamWStep* adam = nullptr) {
  PL_TRY(check_desc(d, true));
  if (!x || !dy || !grads) PL_FAIL(PL_EINVAL, "pl_lifter_bwd: null x/dy/flat_grads");
  // dy: g = dy W5 on skinny.hip stages it as float4, as the forward does x.  x is read by element here (skinny_wide_in_kernel,
  // first_wgrad) or behind launch_gemm_f32's gate; dx leaves through that GEMM's gated epilogue.
  PL_REQUIRE_ALIGNED16("pl_lifter_bwd", dy);
  if (B <= 0) PL_FAIL(PL_ESHAPE, "pl_lifter_bwd: B=%lld", (long long)B);
  const Ws w = plan(d, B);
  PL_TRY(check_ws(w, ws, ws_bytes));
  const ParamLayout P = param_layout(d);
  BwdCtx c = {d, w, P, ws, (hipStream_t)stream, x, dy, dx, grads, (int)B, d->hidden, d->out_dim, l_hi, l_lo};
  c.kscale = eval_bn ? 1.0f : dropout_key(d->p_dropout, 0, 0, 0, nullptr, nullptr).kscale;
  c.eval_bn = eval_bn;
  c.small = !eval_bn && w.bn_small;
  c.sl = !eval_bn && w.small_layer;
  c.top_fused = do_output && !eval_bn && w.top_fused && l_hi == w.L - 1 && l_hi >= l_lo;
  c.loss_out = loss_out;
  c.n_loss_part = n_loss_part;                   // partial sums of the loss in w.mse, their sum times loss_inv_n = the loss
  c.loss_inv_n = loss_inv_n;
  c.adam = adam;
  c.adam_rides = adam && c.top_fused && l_lo == 0 && w.adam_rides;
  if (do_output) PL_TRY(bwd_output(c));
  for (int l = l_hi; l >= l_lo; --l) {
    PL_TRY(bwd_layer_bn(c, l));
    PL_TRY(bwd_layer_linear(c, l));
  }
  if (c.pending.R > 0) c.jobs.push_back(c.pending);       // (slab_sum_rides_below promised a launch that then took it: none is left)
  float inv_n = 0.f;
  uint64_t* tick = nullptr;
  if (loss_out && !c.top_fused) {
    c.job(f32(ws, w.mse), loss_out, c.n_loss_part, 1, 2, 0);
    inv_n = loss_inv_n;
    tick = const_cast<uint64_t*>(d->step_dev);
  }
  if (!c.jobs.empty()) PL_TRY(launch_reduce_rows_multi(c.jobs.data(), (int)c.jobs.size(), inv_n, tick, c.s));
  if (adam) {
    // what no backward launch carried: the bottom of the arena (first layer and the first residual Linear) -- or all of it
    const int64_t n = c.adam_rides ? (w.L > 1 ? P.off[4 * 1 + 1] : P.total) : P.total;
    // (the same fields as ride(); pl_lifter_train_step checked that lr_dev and t_dev go together)
    const AdamWArgs a = {const_cast<float*>(d->params), grads, adam->m, adam->v, n,
                         {adam->lr, adam->beta1, adam->beta2, adam->eps, adam->weight_decay, 1.0f, adam->t, adam->lr_dev,
                          adam->t_dev}, adam->ema};
    PL_TRY(launch_adamw(a, c.s));
  }
  return PL_OK;
}

extern "C" int pl_lifter_bwd(const PLDesc* d, const float* x, const float* dy, int64_t B, void* ws,
                             size_t ws_bytes, float* dx, float* grads, void* stream) {
  if (!d) PL_FAIL(PL_EINVAL, "descriptor is NULL");
  return bwd_impl(d, x, dy, B, ws, ws_bytes, dx, grads, stream, true, 2 * d->num_stage, 0);
}

extern "C" int pl_lifter_bwd_eval(const PLDesc* d, const float* x, const float* dy, int64_t B, void* ws,
                                  size_t ws_bytes, float* dx, float* grads, void* stream) {
  if (!d) PL_FAIL(PL_EINVAL, "descriptor is NULL");
  return bwd_impl(d, x, dy, B, ws, ws_bytes, dx, grads, stream, true, 2 * d->num_stage, 0, true);
}

static int check_range(const PLDesc* d, int hi, int lo, const char* who) {
  const int L = 1 + 2 * d->num_stage;
  if (lo < 0 || hi < lo || hi > L) PL_FAIL(PL_EINVAL, "%s: layer range hi=%d lo=%d outside 0..%d", who, hi, lo, L);
  return PL_OK;
}

extern "C" int pl_lifter_bwd_layers(const PLDesc* d, const float* x, const float* dy, int64_t B, void* ws,
                                    size_t ws_bytes, float* dx, float* grads, int hi, int lo, void* stream) {
  PL_TRY(check_desc(d, true));
  PL_TRY(check_range(d, hi, lo, "pl_lifter_bwd_layers"));
  const int L = 1 + 2 * d->num_stage;
  return bwd_impl(d, x, dy, B, ws, ws_bytes, lo == 0 ? dx : nullptr, grads, stream, hi == L, hi == L ? L - 1 : hi, lo);
}

// ---------------------------------------------------------------------------------------
// GEMM building block (tests)
// ---------------------------------------------------------------------------------------
extern "C" int pl_gemm_f32(int layout, const float* A, const float* Bm, float* C, int64_t M, int64_t N,
                           int64_t K, const float* bias, int split_k, float* slabs, void* stream) {
  return pl_gemm_arith(layout, PL_F32, A, Bm, C, M, N, K, bias, split_k, slabs, stream);
}

extern "C" int pl_gemm_arith(int layout, int arith, const float* A, const float* Bm, float* C, int64_t M,
                             int64_t N, int64_t K, const float* bias, int split_k, float* slabs, void* stream) {
  if (layout < 0 || layout > 2) PL_FAIL(PL_EINVAL, "pl_gemm_f32: layout %d", layout);
  // the PLDtype values and the two test hooks forcing the PL_BF16X6 planes / fragment-split main loop
  if (arith != kArithF32 && arith != kArithBf16 && arith != kArithX6 && arith != kArithX6Planes && arith != kArithX6Frag)
    PL_FAIL(PL_EDTYPE, "pl_gemm_arith: arith %d", arith);
  if (M <= 0 || N <= 0 || K <= 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX)
    PL_FAIL(PL_ESHAPE, "pl_gemm_f32: bad shape");
  GemmArgs g = {};
  g.A = A; g.B = Bm; g.C = C; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.bias = bias;
  g.lda = layout == kTN ? (int)M : (int)K;
  g.ldb = layout == kNT ? (int)K : (int)N;
  g.ldc = (int)N;
  g.split_k = 1;
  g.arith = arith;
  hipStream_t s = (hipStream_t)stream;
  if (split_k > 1) {
    if (layout != kTN || !slabs || bias) PL_FAIL(PL_EINVAL, "pl_gemm_f32: split_k needs layout 2, slabs and no bias");
    g.C = slabs; g.split_k = split_k;
    PL_TRY(launch_gemm_f32(kTN, g, s));
    return launch_reduce_slabs(slabs, split_k, M * N, C, s);
  }
  return launch_gemm_f32((GemmLayout)layout, g, s);
}

// What `mode` means to the planes GEMM: PL_F16X3 is two fp16 planes per operand, whose products carry the caller's static
// (out_scale) and device-side (dyn_inv = {1 / S}) scales; PL_BF16 is one unscaled bf16 plane.
static void set_planes_mode(PlanesGemmArgs& g, int mode, float out_scale, const float* dyn_inv) {
  g.mode = mode == PL_F16X3 ? 2 : 0;
  g.out_scale = mode == PL_F16X3 ? out_scale : 1.0f;
  g.dyn_inv = mode == PL_F16X3 ? dyn_inv : nullptr;
}

// C = op(A) op(B) on 16-bit operand planes: the fp32 operands are split into planes in `scratch` first (the lifter's
// own producers write planes directly), then the planes GEMM of gemm_planes.hip runs.  mode: PL_F16X3 or PL_BF16.
extern "C" size_t pl_gemm_planes_scratch_bytes(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return (size_t)(align_up(M * K * 4, 256) + align_up(N * K * 4, 256));
}

extern "C" int pl_gemm_planes(int layout, int mode, const float* A, const float* Bm, float* C, int64_t M, int64_t N,
                              int64_t K, const float* bias, float scale_a, float scale_b, void* scratch, void* stream) {
  if (layout < 0 || layout > 2) PL_FAIL(PL_EINVAL, "pl_gemm_planes: layout %d", layout);
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "pl_gemm_planes: mode %d", mode);
  if (!A || !Bm || !C || !scratch) PL_FAIL(PL_EINVAL, "pl_gemm_planes: null pointer");
  // A, Bm: split_planes_kernel reads float4; C, bias: the planes GEMM's staged epilogue moves 16 bytes at a time
  PL_REQUIRE_ALIGNED16("pl_gemm_planes", A);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes", Bm);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes", C);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes", bias);
  if (M <= 0 || N <= 0 || K <= 0 || M * K >= (1ll << 29) || N * K >= (1ll << 29)) PL_FAIL(PL_ESHAPE, "pl_gemm_planes: bad shape");
  if (!(scale_a > 0.f) || !(scale_b > 0.f)) PL_FAIL(PL_EINVAL, "pl_gemm_planes: scales must be positive powers of two");
  hipStream_t s = (hipStream_t)stream;
  unsigned short* pa = static_cast<unsigned short*>(scratch);
  unsigned short* pb = reinterpret_cast<unsigned short*>(static_cast<char*>(scratch) + align_up(M * K * 4, 256));
  const int kind = mode == PL_F16X3 ? 2 : 1;
  PlaneOut oa = {pa, pa + M * K, scale_a, nullptr, kind}, ob = {pb, pb + N * K, scale_b, nullptr, kind};
  range_watch(oa, PL_RANGE_SITE_SPLIT); range_watch(ob, PL_RANGE_SITE_SPLIT);
  PL_TRY(launch_split_planes(A, M * K, oa, s));
  PL_TRY(launch_split_planes(Bm, N * K, ob, s));
  PlanesGemmArgs g = {};
  g.A = pa; g.B = pb; g.a_plane = M * K; g.b_plane = N * K;
  g.lda = layout == kTN ? (int)M : (int)K;
  g.ldb = layout == kNT ? (int)K : (int)N;
  set_planes_mode(g, mode, 1.0f / (scale_a * scale_b), nullptr);
  g.e.C = C; g.e.M = (int)M; g.e.N = (int)N; g.e.K = (int)K; g.e.ldc = (int)N; g.e.split_k = 1; g.e.bias = bias;
  return launch_gemm_planes((GemmLayout)layout, g, s);
}

// K slices of a planes GEMM with few output tiles (the conv weight gradients: K = pixels): enough workgroups for every
// CU twice, slices of whole 32-k tiles, at most 64 slabs -- 128 where the output is small enough for the slab reduce not to
// matter (the stem's weight gradient: 64 x 224 outputs, 2 tiles, 4.2 M pixels: 128 workgroups took 1.49 ms, 256 take half)
extern "C" int pl_gemm_planes_splits(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const int cap = M * N <= 32768 ? 128 : 64;
  int s = 1;
  while (s < cap && tiles * s < 512 && K % (32 * 2 * s) == 0 && K / (2 * s) >= 256) s *= 2;
  return s;
}

// The launch of a planes GEMM into C [M][N], over pl_gemm_planes_splits(M, N, K) K slices: more than one go to `slabs` and are
// summed into C by a second launch (no bias or epilogue statistics then).  g.e holds M, N, K, ldc and any bias / statistics.
static int launch_planes_split_k(const char* who, GemmLayout layout, PlanesGemmArgs& g, float* C, float* slabs, hipStream_t s) {
  const int splits = pl_gemm_planes_splits(g.e.M, g.e.N, g.e.K);
  if (splits > 1) {
    if (!slabs) PL_FAIL(PL_EWORKSPACE, "%s: %d K slices need slabs", who, splits);
    if (g.e.bias || g.e.stat_sum) PL_FAIL(PL_EINVAL, "%s: no bias / statistics on a split-K problem", who);
    g.e.C = slabs; g.e.split_k = splits;
    PL_TRY(launch_gemm_planes(layout, g, s));
    return launch_reduce_slabs(slabs, splits, (int64_t)g.e.M * g.e.N, C, s);
  }
  g.e.C = C; g.e.split_k = 1;
  return launch_gemm_planes(layout, g, s);
}

extern "C" int pl_gemm_planes_raw(int layout, int mode, const void* A, int64_t a_plane, int64_t lda, const void* Bm,
                                  int64_t b_plane, int64_t ldb, float* C, int64_t M, int64_t N, int64_t K, const float* bias,
                                  float out_scale, const float* dyn_inv, float* slabs, float* stat, void* stream) {
  if (layout < 0 || layout > 2) PL_FAIL(PL_EINVAL, "pl_gemm_planes_raw: layout %d", layout);
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "pl_gemm_planes_raw: mode %d", mode);
  if (!A || !Bm || !C) PL_FAIL(PL_EINVAL, "pl_gemm_planes_raw: null pointer");
  PL_REQUIRE_ALIGNED16("pl_gemm_planes_raw", A);             // (operand planes: 16-byte LDS-DMA; C, bias, stat: the staged epilogue)
  PL_REQUIRE_ALIGNED16("pl_gemm_planes_raw", Bm);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes_raw", C);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes_raw", bias);
  PL_REQUIRE_ALIGNED16("pl_gemm_planes_raw", stat);
  if (M <= 0 || N <= 0 || K <= 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX || lda > INT32_MAX || ldb > INT32_MAX)
    PL_FAIL(PL_ESHAPE, "pl_gemm_planes_raw: bad shape");
  PlanesGemmArgs g = {};
  g.A = static_cast<const unsigned short*>(A); g.B = static_cast<const unsigned short*>(Bm);
  g.a_plane = a_plane; g.b_plane = b_plane; g.lda = (int)lda; g.ldb = (int)ldb;
  set_planes_mode(g, mode, out_scale, dyn_inv);
  g.e.M = (int)M; g.e.N = (int)N; g.e.K = (int)K; g.e.ldc = (int)N; g.e.bias = bias;
  if (stat) { g.e.stat_sum = stat; g.e.stat_m2 = stat + (size_t)gemm_stat_groups((int)M) * N; }
  return launch_planes_split_k("pl_gemm_planes_raw", (GemmLayout)layout, g, C, slabs, (hipStream_t)stream);
}

extern "C" int pl_gemm_stat_groups(int64_t M) { return M > 0 && M <= INT32_MAX ? gemm_stat_groups((int)M) : 0; }

// KxK convolutions on the planes GEMM with the input gathered by the loader waves (implicit GEMM, gemm_planes16.h)
static int conv_planes_geom(GemmArgs& e, int64_t B, int64_t H, int64_t W, int64_t Cin, int KH, int KW, int stride, int pad,
                            int64_t* Ho, int64_t* Wo, const char* who, int stride_w = 0, int pad_w = -1, int pad_w_right = -1) {
  if (stride_w <= 0) stride_w = stride;
  if (pad_w < 0) pad_w = pad;
  if (pad_w_right < 0) pad_w_right = pad_w;          // (the gather pads by its bounds test: only Wo knows the right padding)
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
    PL_FAIL(PL_ESHAPE, "%s: bad geometry", who);
  *Ho = (H + 2 * pad - KH) / stride + 1;
  *Wo = (W + pad_w + pad_w_right - KW) / stride_w + 1;
  if (*Ho <= 0 || *Wo <= 0 || B * *Ho * *Wo > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: bad geometry", who);
  e.conv_cin = (int)Cin; e.conv_h = (int)H; e.conv_w = (int)W; e.conv_ho = (int)*Ho; e.conv_wo = (int)*Wo;
  e.conv_kw = KW; e.conv_stride = stride; e.conv_stride_w = stride_w; e.conv_pad_h = pad; e.conv_pad_w = pad_w;
  return PL_OK;
}

// the folded eval-mode epilogue and the planes output of a planes convolution (PLPlanesEpilogue)
static int apply_planes_epilogue(GemmArgs& e, int mode, const PLPlanesEpilogue* ep, int64_t n_out, const char* who) {
  if (!ep) return PL_OK;
  if ((ep->scale != nullptr) != (ep->shift != nullptr)) PL_FAIL(PL_EINVAL, "%s: scale without shift", who);
  if (ep->relu < 0 || ep->relu > 2) PL_FAIL(PL_EINVAL, "%s: relu %d", who, ep->relu);
  e.bias = ep->bias; e.col_scale = ep->scale; e.col_shift = ep->shift; e.resid = ep->resid; e.relu = ep->relu;
  if (ep->y_planes) {
    if ((reinterpret_cast<uintptr_t>(ep->y_planes) & 15) || (n_out & 7)) PL_FAIL(PL_EINVAL, "%s: y_planes misaligned", who);
    e.cpl_h = static_cast<unsigned short*>(ep->y_planes);
    e.cpl_l = e.cpl_h + n_out;
    e.cpl_scale = kConvActPlaneScale;
    e.cpl_kind = mode == PL_F16X3 ? 2 : 1;
    e.cpl_range = e.cpl_kind == 2 ? range_record() : nullptr; e.cpl_site = PL_RANGE_SITE_CONV_ACT;
  }
  return PL_OK;
}

// The gathered forward behind pl_conv2d_planes_fwd[_ep][_hw] (`who`: the name the caller's errors carry).  The training
// forms pass dyn_inv / stat and no epilogue, the eval forms an epilogue (with which y may be NULL: planes output only).
static int conv_planes_fwd(const char* who, int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                           int64_t Cin, const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride_h,
                           int stride_w, int pad_h, int pad_w, int pad_w_right, float* y, float out_scale, const float* dyn_inv,
                           float* stat, const PLPlanesEpilogue* ep, void* stream) {
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "%s: mode %d", who, mode);
  if (!x_planes || !w_planes || (!y && !(ep && ep->y_planes)) || Cout <= 0) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PlanesGemmArgs g = {};
  int64_t Ho, Wo;
  PL_TRY(conv_planes_geom(g.e, B, H, W, Cin, KH, KW, stride_h, pad_h, &Ho, &Wo, who, stride_w, pad_w, pad_w_right));
  const int64_t K = (int64_t)KH * KW * Cin;
  g.A = static_cast<const unsigned short*>(x_planes); g.B = static_cast<const unsigned short*>(w_planes);
  g.a_plane = x_plane; g.b_plane = w_plane; g.lda = 0; g.ldb = (int)K;
  set_planes_mode(g, mode, out_scale, dyn_inv);
  g.e.C = y; g.e.M = (int)(B * Ho * Wo); g.e.N = (int)Cout; g.e.K = (int)K; g.e.ldc = (int)Cout; g.e.split_k = 1;
  if (stat) { g.e.stat_sum = stat; g.e.stat_m2 = stat + (size_t)gemm_stat_groups(g.e.M) * Cout; }
  PL_TRY(apply_planes_epilogue(g.e, mode, ep, B * Ho * Wo * Cout, who));
  return launch_gemm_planes(kNT, g, (hipStream_t)stream);
}

extern "C" int pl_conv2d_planes_fwd(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin,
                                    const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW, int stride, int pad,
                                    float* y, float out_scale, const float* dyn_inv, float* stat, void* stream) {
  return conv_planes_fwd("pl_conv2d_planes_fwd", mode, x_planes, x_plane, B, H, W, Cin, w_planes, w_plane, Cout, KH, KW, stride,
                         stride, pad, pad, pad, y, out_scale, dyn_inv, stat, nullptr, stream);
}

extern "C" int pl_conv2d_planes_fwd_hw(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                       int64_t Cin, const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW,
                                       int stride_h, int stride_w, int pad_h, int pad_w, int pad_w_right, float* y,
                                       float out_scale, const float* dyn_inv, float* stat, void* stream) {
  return conv_planes_fwd("pl_conv2d_planes_fwd", mode, x_planes, x_plane, B, H, W, Cin, w_planes, w_plane, Cout, KH, KW, stride_h,
                         stride_w, pad_h, pad_w, pad_w_right, y, out_scale, dyn_inv, stat, nullptr, stream);
}

extern "C" int pl_conv2d_planes_fwd_ep(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                       int64_t Cin, const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW,
                                       int stride, int pad, float* y, float out_scale, const PLPlanesEpilogue* ep, void* stream) {
  return conv_planes_fwd("pl_conv2d_planes_fwd_ep", mode, x_planes, x_plane, B, H, W, Cin, w_planes, w_plane, Cout, KH, KW, stride,
                         stride, pad, pad, pad, y, out_scale, nullptr, nullptr, ep, stream);
}

extern "C" int pl_conv2d_planes_fwd_ep_hw(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                          int64_t Cin, const void* w_planes, int64_t w_plane, int64_t Cout, int KH, int KW,
                                          int stride_h, int stride_w, int pad_h, int pad_w, int pad_w_right, float* y,
                                          float out_scale, const PLPlanesEpilogue* ep, void* stream) {
  return conv_planes_fwd("pl_conv2d_planes_fwd_ep", mode, x_planes, x_plane, B, H, W, Cin, w_planes, w_plane, Cout, KH, KW,
                         stride_h, stride_w, pad_h, pad_w, pad_w_right, y, out_scale, nullptr, nullptr, ep, stream);
}

// nn.ConvTranspose2d(4, 2, 1, bias=False) forward on the planes GEMM: four 2x2-tap convolutions at the INPUT resolution,
// one per output parity (no zero insertion), each storing straight into its pixels of y [B][2H][2W][Cout].
// wsub_planes: planes of conv.deconv_subkernels(weight) = [4 parities][Cout][2][2][Cin].
// The launcher behind pl_deconv4x4s2_planes_fwd (dyn_inv, no epilogue) and _fwd_ep (an epilogue; y may then be NULL).
static int deconv_planes_fwd(const char* who, int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                             int64_t Cin, const void* wsub_planes, int64_t wsub_plane, int64_t Cout, float* y, float out_scale,
                             const float* dyn_inv, const PLPlanesEpilogue* ep, void* stream) {
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "%s: mode %d", who, mode);
  if (!x_planes || !wsub_planes || (!y && !(ep && ep->y_planes)) || Cout <= 0) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || B * H * W > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: bad geometry", who);
  if (ep && ep->resid) PL_FAIL(PL_EINVAL, "%s: no residual on a transposed convolution", who);
  const int64_t K = 4 * Cin, nsub = Cout * K;
  for (int ph = 0; ph < 2; ++ph)
    for (int pw = 0; pw < 2; ++pw) {
      PlanesGemmArgs g = {};
      g.e.conv_cin = (int)Cin; g.e.conv_h = (int)H; g.e.conv_w = (int)W; g.e.conv_ho = (int)H; g.e.conv_wo = (int)W;
      g.e.conv_kw = 2; g.e.conv_stride = 1;
      g.e.conv_pad_h = ph ? 0 : 1; g.e.conv_pad_w = pw ? 0 : 1;      // even outputs: taps from rows a-1, a; odd: a, a+1
      g.e.scat_on = 1; g.e.scat_ph = ph; g.e.scat_pw = pw;
      g.A = static_cast<const unsigned short*>(x_planes);
      g.B = static_cast<const unsigned short*>(wsub_planes) + (size_t)(ph * 2 + pw) * nsub;
      g.a_plane = x_plane; g.b_plane = wsub_plane; g.lda = 0; g.ldb = (int)K;
      set_planes_mode(g, mode, out_scale, dyn_inv);
      g.e.C = y; g.e.M = (int)(B * H * W); g.e.N = (int)Cout; g.e.K = (int)K; g.e.ldc = (int)Cout; g.e.split_k = 1;
      PL_TRY(apply_planes_epilogue(g.e, mode, ep, B * 4 * H * W * Cout, who));   // (its checks: before the first launch)
      PL_TRY(launch_gemm_planes(kNT, g, (hipStream_t)stream));
    }
  return PL_OK;
}

extern "C" int pl_deconv4x4s2_planes_fwd_ep(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                            int64_t Cin, const void* wsub_planes, int64_t wsub_plane, int64_t Cout, float* y,
                                            float out_scale, const PLPlanesEpilogue* ep, void* stream) {
  return deconv_planes_fwd("pl_deconv4x4s2_planes_fwd_ep", mode, x_planes, x_plane, B, H, W, Cin, wsub_planes, wsub_plane, Cout, y,
                           out_scale, nullptr, ep, stream);
}

extern "C" int pl_deconv4x4s2_planes_fwd(int mode, const void* x_planes, int64_t x_plane, int64_t B, int64_t H, int64_t W,
                                         int64_t Cin, const void* wsub_planes, int64_t wsub_plane, int64_t Cout, float* y,
                                         float out_scale, const float* dyn_inv, void* stream) {
  return deconv_planes_fwd("pl_deconv4x4s2_planes_fwd", mode, x_planes, x_plane, B, H, W, Cin, wsub_planes, wsub_plane, Cout, y,
                           out_scale, dyn_inv, nullptr, stream);
}

extern "C" int pl_conv2d_planes_wgrad(int mode, const void* dz_planes, int64_t dz_plane, const void* x_planes, int64_t x_plane,
                                      int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH, int KW, int stride,
                                      int pad, float* dw, float out_scale, const float* dyn_inv, float* slabs, void* stream) {
  return pl_conv2d_planes_wgrad_hw(mode, dz_planes, dz_plane, x_planes, x_plane, B, H, W, Cin, Cout, KH, KW, stride, stride, pad,
                                   pad, pad, dw, out_scale, dyn_inv, slabs, stream);
}

extern "C" int pl_conv2d_planes_wgrad_hw(int mode, const void* dz_planes, int64_t dz_plane, const void* x_planes,
                                         int64_t x_plane, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int KH,
                                         int KW, int stride_h, int stride_w, int pad_h, int pad_w, int pad_w_right, float* dw,
                                         float out_scale, const float* dyn_inv, float* slabs, void* stream) {
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "pl_conv2d_planes_wgrad: mode %d", mode);
  if (!dz_planes || !x_planes || !dw || Cout <= 0) PL_FAIL(PL_EINVAL, "pl_conv2d_planes_wgrad: null pointer");
  PlanesGemmArgs g = {};
  int64_t Ho, Wo;
  PL_TRY(conv_planes_geom(g.e, B, H, W, Cin, KH, KW, stride_h, pad_h, &Ho, &Wo, "pl_conv2d_planes_wgrad", stride_w, pad_w, pad_w_right));
  const int64_t N = (int64_t)KH * KW * Cin, K = B * Ho * Wo;
  g.A = static_cast<const unsigned short*>(dz_planes); g.B = static_cast<const unsigned short*>(x_planes);
  g.a_plane = dz_plane; g.b_plane = x_plane; g.lda = (int)Cout; g.ldb = 0;
  set_planes_mode(g, mode, out_scale, dyn_inv);
  g.e.M = (int)Cout; g.e.N = (int)N; g.e.K = (int)K; g.e.ldc = (int)N;
  return launch_planes_split_k("pl_conv2d_planes_wgrad", kTN, g, dw, slabs, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// measurement hook (bench.py): per-launch GEMM durations from HIP events on the launch stream
// ---------------------------------------------------------------------------------------
extern "C" int pl_prof_enable(int on) { return prof_enable(on); }
extern "C" int pl_prof_read(double min_flops, double max_flops, double* ms_total, int64_t* launches,
                            double* flops_total) {
  if (!ms_total || !launches || !flops_total) PL_FAIL(PL_EINVAL, "pl_prof_read: null pointer");
  return prof_read(min_flops, max_flops, ms_total, launches, flops_total);
}

// ---------------------------------------------------------------------------------------
// fused train step: forward (training mode) + MSE(mean) + backward in one call
// ---------------------------------------------------------------------------------------
static int train_fwd_bwd_impl(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws, size_t ws_bytes,
                              uint64_t seed, uint64_t step, const PLCriterion* crit, float* y, float* loss, float* grads, int hi,
                              int lo, void* stream, const PLAdamWStep* adam);

extern "C" int pl_lifter_train_fwd_bwd_crit(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws,
                                            size_t ws_bytes, uint64_t seed, uint64_t step, const PLCriterion* crit, float* y,
                                            float* loss, float* grads, int hi, int lo, void* stream) {
  return train_fwd_bwd_impl(d, x, target, B, ws, ws_bytes, seed, step, crit, y, loss, grads, hi, lo, stream, nullptr);
}
extern "C" int pl_lifter_train_fwd_bwd(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws,
                                       size_t ws_bytes, uint64_t seed, uint64_t step, float* y, float* loss,
                                       float* grads, int hi, int lo, void* stream) {
  return pl_lifter_train_fwd_bwd_crit(d, x, target, B, ws, ws_bytes, seed, step, nullptr, y, loss, grads, hi, lo, stream);
}

extern "C" int pl_lifter_step_carries_adamw(const PLDesc* d, int64_t B) {
  PL_TRY(check_desc(d, false));
  return B > 0 && plan(d, B).adam_rides ? 1 : 0;
}

extern "C" int pl_lifter_bwd_slab_rides(const PLDesc* d, int64_t B, int hi, int lo) {
  PL_TRY(check_desc(d, false));
  PL_TRY(check_range(d, hi, lo, "pl_lifter_bwd_slab_rides"));
  if (B <= 0 || B > INT32_MAX) return 0;
  const Ws w = plan(d, B);
  int n = 0;
  for (int l = hi < w.L ? hi : w.L - 1; l > lo; --l) n += pl::slab_sum_rides_below(w, d->hidden, (int)B, l, lo) ? 1 : 0;
  return n;
}

extern "C" int pl_lifter_train_step_crit(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws,
                                         size_t ws_bytes, uint64_t seed, uint64_t step, const PLCriterion* crit, float* y,
                                         float* loss, float* grads, const PLAdamWStep* opt, void* stream) {
  if (!opt || !opt->m || !opt->v || (opt->lr_dev != nullptr) != (opt->t_dev != nullptr) || opt->t < (opt->t_dev ? 0 : 1))
    PL_FAIL(PL_EINVAL, "pl_lifter_train_step: bad optimizer description");
  if (opt->ema) PL_TRY(check_ema(*opt->ema, "pl_lifter_train_step"));
  if (!d) PL_FAIL(PL_EINVAL, "descriptor is NULL");
  return train_fwd_bwd_impl(d, x, target, B, ws, ws_bytes, seed, step, crit, y, loss, grads, 1 + 2 * d->num_stage, 0, stream, opt);
}
extern "C" int pl_lifter_train_step(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws, size_t ws_bytes,
                                    uint64_t seed, uint64_t step, float* y, float* loss, float* grads, const PLAdamWStep* opt,
                                    void* stream) {
  return pl_lifter_train_step_crit(d, x, target, B, ws, ws_bytes, seed, step, nullptr, y, loss, grads, opt, stream);
}

static int train_fwd_bwd_impl(const PLDesc* d, const float* x, const float* target, int64_t B, void* ws, size_t ws_bytes,
                              uint64_t seed, uint64_t step, const PLCriterion* crit, float* y, float* loss, float* grads, int hi,
                              int lo, void* stream, const PLAdamWStep* adam) {
  PL_TRY(check_desc(d, true));
  if (!x || !target || !y || !loss || !grads) PL_FAIL(PL_EINVAL, "pl_lifter_train_fwd_bwd: null pointer");
  PL_REQUIRE_ALIGNED16("pl_lifter_train_fwd_bwd", x);        // (target, y and loss: element kernels only -- criterion.hip, small_layer.hip)
  if (B <= 0) PL_FAIL(PL_ESHAPE, "pl_lifter_train_fwd_bwd: B=%lld", (long long)B);
  PL_TRY(check_range(d, hi, lo, "pl_lifter_train_fwd_bwd"));
  Crit cr;
  PL_TRY(crit_resolve(crit, B, d->out_dim, cr, "pl_lifter_train_fwd_bwd"));
  const Ws w = plan(d, B);
  PL_TRY(check_ws(w, ws, ws_bytes));
  float* dy = f32(ws, w.dyout);
  const int L = 1 + 2 * d->num_stage;
  // the partial sums the loss pass of this route leaves in w.mse, and what their sum is multiplied by
  int n_part = w.loss == Loss::SmallMse ? small_loss_partials(cr, (int)B, d->out_dim)
               : w.loss == Loss::FromSlabs ? loss_partials(Crit{}, B, d->out_dim) : loss_partials(cr, B, d->out_dim);
  if (hi == L && w.loss == Loss::PartialOnly) {
    PL_TRY(pl_lifter_fwd_train(d, x, y, B, ws, ws_bytes, seed, step, nullptr, stream));
    PL_TRY(loss_partial_only(y, target, B, d->out_dim, cr, 1.0f, dy, f32(ws, w.mse), stream, "pl_lifter_train_fwd_bwd"));
  } else if (hi == L) {
    // the forward leaves the output Linear's slabs, the MSE pass adds them up
    const int H = d->hidden, O = d->out_dim;
    PL_TRY(fwd_saved_impl(d, x, y, B, ws, ws_bytes, seed, step, nullptr, stream, false, true));
    const float* bias = d->params + param_layout(d).off[4 * L + 1];
    if (w.loss == Loss::SmallMse) {
      SmallHeadArgs h = {};
      h.ypart = f32(ws, w.slabs); h.NS = H / 16; h.B = (int)B; h.O = O; h.bias = bias; h.y = y;
      h.tgt = target; h.grad_scale = 1.0f; h.dpred = dy; h.mpart = f32(ws, w.mse); h.crit = cr;
      PL_TRY(launch_small_mse(h, (hipStream_t)stream));
    } else
      PL_TRY(loss_partial_from_slabs(f32(ws, w.slabs), skinny_narrow_out_splits((int)B, H), (int)B, O, bias, target, cr, 1.0f, y,
                                     dy, f32(ws, w.mse), stream));
  }
  if (hi == L && cr.has_sk) {
    // the skeleton terms, on every route the same launch: y, dy and the route's partials are in memory; it adds into dy and
    // appends its own partials, which the route's finaliser sums with the rest
    PL_TRY(launch_skeleton_terms(cr, y, target, B, d->out_dim, 1.0f, crit_inv_n(cr, B * d->out_dim), dy, f32(ws, w.mse) + n_part,
                                 stream, "pl_lifter_train_fwd_bwd"));
    n_part += skeleton_partials(B);
  }
  return bwd_impl(d, x, dy, B, ws, ws_bytes, nullptr, grads, stream, hi == L, hi == L ? L - 1 : hi, lo, false,
                  hi == L ? loss : nullptr, n_part, crit_inv_n(cr, B * d->out_dim), adam);
}
