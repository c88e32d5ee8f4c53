// "Planes in HBM" GEMM: shared declarations of the main loops in gemm_planes16.h.  Operands arrive PRE-SPLIT as 16-bit
// planes, written once by the kernel that produces the tensor (bn_apply, bn_bwd_dz, adamw, ...), never split inside the GEMM.
//
// A plane tensor is [NPL][rows][cols], row-major, plane stride given in elements.  What this buys over the round-1 loop
// (fp32 operands through registers, split on the vector ALU, ds_write):
//   * global -> LDS by buffer_load_dwordx4 ... lds (LDS-DMA): no VGPR round trip, no ds_write, no split VALU --
//     the inner loop is ds_read + MFMA;
//   * LDS stages with the DMA of later tiles in flight across the one barrier per tile (counted vmcnt, raw s_barrier:
//     __syncthreads() would drain the DMA queue);
//   * k-contiguous operands XOR-swizzled on the SOURCE address so that the fragment reads are bank-conflict free (the DMA
//     writes LDS linearly: lane -> base + 16*lane); k-strided operands (dW = dz^T a, dX = dz W) read with the hardware
//     transpose ds_read_b64_tr_b16 -- no transposed copy in HBM or LDS.
// (The 32x32x16 form of the loop was removed once the 16x16x32 one had replaced it everywhere; it is in git history.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace plp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// Arithmetic modes of the planes GEMM (what the 16-bit planes hold and which products are accumulated):
//   kBf16    1 bf16 plane : a*b on the rounded operands (PL_BF16; bf16 STORAGE of activations and weights)
//   kBf16x6  3 bf16 planes: x = x0 + x1 + x2 exactly; a0b0 + a0b1 + a1b0 + a0b2 + a1b1 + a2b0, one accumulator
//   kF16x3   2 fp16 planes: S x = h + l / 2048 with h = fp16(S x), l = fp16((S x - h) * 2048), S a per-tensor power
//            of two that keeps h in fp16's normal range (22-23 significant bits); a*b = h_a h_b + (h_a l_b +
//            l_a h_b) / 2048 on TWO accumulators (main, low), combined and un-scaled in the epilogue.  The dropped
//            l_a l_b term is < 2^-22 |ab|.  Three MFMAs per product term instead of six: on a chip whose matrix
//            clock under load makes six-product bf16 MFMA-bound (measured: 40 us for 51.5 GFLOP issued), this
//            halves the bound.  Error against fp64 on the golden eval forward: 6.4e-5 mm (exact products 6.0e-5,
//            bf16x6 5.9e-5) -- indistinguishable; the fp32 accumulation of either is what sets the floor.
enum PlanesMode { kBf16 = 0, kBf16x6 = 1, kF16x3 = 2 };
template <int MODE> struct ModeCfg;
template <> struct ModeCfg<kBf16>   { static constexpr int NPL = 1, NACC = 1, NPROD = 1; };
template <> struct ModeCfg<kBf16x6> { static constexpr int NPL = 3, NACC = 1, NPROD = 6; };
template <> struct ModeCfg<kF16x3>  { static constexpr int NPL = 2, NACC = 2, NPROD = 3; };
constexpr float kF16LoScale = 2048.0f;      // l is stored times 2^11

struct PlanesArgs {
  const __bf16* A;   // planes of A: k-contiguous [M][K] (lda = K) or k-strided [K][M] (lda = M)
  const __bf16* B;   // planes of B: k-contiguous [N][K] (ldb = K) or k-strided [K][N] (ldb = N)
  float* C;
  int M, N, K;
  int lda, ldb, ldc;
  int split_k;       // > 1: slice z covers K/split_k and writes C + z*M*ldc
  size_t a_plane, b_plane;   // elements between two planes
  // Implicit-GEMM convolution (16x16x32 loop; cv_cin == 0: none).  The gathered operand is the NHWC tensor x
  // [B][cv_h][cv_w][cv_cin] (planes), every 32-k tile inside ONE filter tap (cv_cin % 32 == 0), padding pixels read as
  // zeros (an out-of-range LDS-DMA lane writes zeros: tools/ubench/dma_oob_probe.hip):
  //   forward / data gradient (NT, gathered A): A = x, row m = output pixel (b, oh, ow), k = (kh*cv_kw + kw)*cv_cin + ci;
  //   weight gradient (TN, gathered B):          B = x, k = output pixel, column n = (kh*cv_kw + kw)*cv_cin + ci.
  // cv_stride: the stride along h, cv_stride_w along w (the stem's pixel-pair view has 2 and 1).  cv_cin == 8 (forward only:
  // cv_kw % 4 == 0): a 32-k tile is four neighbouring taps of one kernel row, 8 channels each.
  int cv_cin, cv_h, cv_w, cv_ho, cv_wo, cv_kw, cv_stride, cv_stride_w, cv_pad_h, cv_pad_w;
};

// A split-K sum that rides on the loader waves of a chained launch (gemm_planes16.h SLAB RIDE): out[i] = ((s0[i] + s1[i]) +
// s2[i]) + s3[i] over n4 float4, slab r at part + r * stride floats.  part == NULL: no ride.
struct SlabRide {
  const float* part;
  float* out;
  long long stride;
  int R, n4;
};

template <int BKX, int NPL, int NST = 3>
struct PlanesCfg {
  static constexpr int OPP = 128 * BKX * 2;     // one plane of one operand tile, bytes
  static constexpr int STAGE = 2 * NPL * OPP;   // A planes then B planes
  static constexpr int LDS = NST * STAGE;
  static constexpr int NJ = BKX / 16;           // DMA instructions per wave, plane and operand tile (1 KiB each)
  static constexpr int NDMA = 2 * NPL * NJ;     // per wave and K tile
};

// 16 bytes per lane, global -> LDS, no VGPR destination: LDS address = lp (wave-uniform) + 16 * lane
#define PLP_BLDS16(rsrc, lp, voff, soff) \
  __builtin_amdgcn_raw_ptr_buffer_load_lds((rsrc), (__attribute__((address_space(3))) void*)(lp), 16, (voff), (soff), 0, 0)

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Issue order of one half step (a single basic block): MFMA, 2 fragment reads, MFMA, 2 reads, ... then MFMA, 1 DMA,
// MFMA, 1 DMA, ...: the matrix pipe never waits for a burst of memory instructions to issue.
template <int NDS, int NVM, int NMF>
__device__ __forceinline__ void sched_half() {
  constexpr int QV0 = (NDS + 1) / 2;   // first MFMA slot that carries a DMA issue
#pragma unroll
  for (int q = 0; q < NMF; ++q) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (2 * q < NDS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    if (q >= QV0 && q < QV0 + NVM) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
  // whatever did not fit under the MFMAs (NPL = 1: four MFMAs per half)
  if (2 * NMF < NDS) __builtin_amdgcn_sched_group_barrier(0x100, NDS - 2 * NMF, 0);
  if (QV0 + NVM > NMF && NVM > 0) __builtin_amdgcn_sched_group_barrier(0x010, NVM, 0);
}

}  // namespace plp
