// What the GEMM kernels of gemm.hip share on the device side: operand images in LDS and their staging, fragment addresses, the
// k-steps, the accumulator layout and the stores that follow from it.  Included by gemm.hip only.  Every function is inlined
// into a kernel and none of it may move a kernel's MFMA loop, change a wait count or add a register spill: tools/isa_diff.py and
// tools/isa_mix.py against the parent commit are the check, profiles/gemm_tile_isa.md the record.
//
// The contracts, stated here and nowhere else:
//
// NT operand image (both operands K-contiguous): [rows][BKT bf16], BKT = 64 (128-byte rows) or 32 (64-byte rows).  The 16-byte
//   chunk c of row r lives at chunk position c ^ gl_sw<BKT>(r): a 16-lane group of ds_read_b128 (16 distinct rows, same logical
//   chunk) then covers all 64 banks exactly once.  The image is filled by global_load_lds_dwordx4, whose LDS destination is
//   linear (wave base + lane * 16 B), so the XOR is applied to the per-lane SOURCE address (chunk position p of the image
//   receives logical chunk (p % CH) ^ gl_sw(p / CH)) and again on the fragment reads.
// Weight-gradient operand image (both operands reduction-major): [r][ROW_ELEMS columns], ROW_ELEMS = 128 or 256.  Chunk c of
//   row r lives at chunk position c ^ (4 * (r & 3)): the four rows of one transposed 4 x 16 read (ds_read_b64_tr_b16) then sit
//   in four different 64-byte bank quarters.  Filled the same way, XOR on the source.
// Zero-block rule (weight gradient, 128- and 256-row tiles): a chunk whose row lies past the end of the row split, or whose
//   column lies past N / K, is fetched from the 16-byte zero block g_zero16 instead: every wave issues every load of every stage
//   (the counted vmcnt waits rely on it) and the product of a chunk that does not exist is zero.
// Accumulator (v_mfma_f32_32x32x16_bf16, D = A.B): of a 32 x 32 block a lane holds COLUMN l31 = lane & 31 (the B operand's row)
//   and, in register r, ROW acc_row(r, lh) = (r & 3) + 8 * (r >> 2) + 4 * lh with lh = lane >> 5 (the A operand's rows).  The NT
//   persistent kernels swap the operands (C^T = B.A^T): lane = row of C, registers 4q .. 4q + 3 = columns 8q + 4lh .. + 3.
#pragma once
#include "common.h"
#include "gemm_plan.h"          // tile geometry: BM2, BN, BR

typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));

template <int BKT> __device__ __forceinline__ int gl_sw(int r) { return BKT == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3); }
__device__ __forceinline__ int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

__device__ __forceinline__ void lds_dma16(const u16* src, u16* dst) {          // one global_load_lds_dwordx4 of a wave
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
__device__ __forceinline__ unsigned lds_addr(const u16* p) { return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const u16*)p; }

template <int NJ>
__device__ __forceinline__ void acc_clear(f32x16 (&acc)[2][NJ]) {
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
}

// A wave's 64 x 64 block (wave row wm, wave column wn) into the fp32 C tile in LDS (row-major, 128 columns): lane = column,
// register = row, the first half of the epilogue through LDS.
__device__ __forceinline__ void acc_to_lds_tile(const f32x16 (&acc)[2][2], float* __restrict__ cs, int wm, int wn, int l31, int lh) {
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) cs[(wm * 64 + i * 32 + acc_row(r, lh)) * 128 + wn * 64 + j * 32 + l31] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------------------
// NT: the stage of the 256 x 128 x 64 kernels (8 waves): A image [256][64] then B image [128][64], 4 + 2 loads per wave.
// ---------------------------------------------------------------------------------------------------------
struct nt256_image {
  static constexpr int STAGE = (BM2 + BN) * 64;          // elements per stage
  int wave, lane;
  const u16* ga[4];
  const u16* gb[2];
  // the tile's source pointers.  A rows past M are clamped to the last row (loaded and computed, never stored); b_row(r) is the
  // row of B behind row r of the B image.
  template <typename BROW>
  __device__ __forceinline__ void set_tile(const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, int M, int m0, BROW b_row) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int p = (i * 8 + wave) * 64 + lane, r = p >> 3, c = (p & 7) ^ gl_sw<64>(r);
      int ra = m0 + r; if (ra > M - 1) ra = M - 1;
      ga[i] = A + (int64_t)ra * lda + c * 8;
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int p = (i * 8 + wave) * 64 + lane, r = p >> 3, c = (p & 7) ^ gl_sw<64>(r);
      gb[i] = B + (int64_t)b_row(r) * ldb + c * 8;
    }
  }
  // k-step k0 into stage slot st of the ring at lds (an argument: kept as a member, the generic pointer cost gemm_nt_256_kernel
  // registers and gemm_nt_persist_kernel four spills)
  __device__ __forceinline__ void stage(u16* lds, int k0, int st) const {
    u16* base = lds + st * STAGE;
#pragma unroll
    for (int i = 0; i < 4; i++) lds_dma16(ga[i] + k0, base + (i * 8 + wave) * 512);
#pragma unroll
    for (int i = 0; i < 2; i++) lds_dma16(gb[i] + k0, base + BM2 * 64 + (i * 8 + wave) * 512);
  }
};

// One k-step of 64 of a wavefront's 64x64 sub-tile: 4 k16-steps of 2x2 MFMA 32x32x16.  The fragment reads are
// inline asm with hand-counted lgkmcnt so that the reads of step ks+1 are in flight while the MFMAs of step ks
// issue (hipcc otherwise re-uses one register set and waits lgkmcnt(0) in front of every group of 4 MFMAs).
// Byte address of (row r, k16-step ks): P ^ (32*ks) with P = tile_base + r*128 + 16*(lh ^ swizzle(r)); the XOR
// form holds because every base is a multiple of 128 bytes.
struct NtFragAddr { unsigned a[2], b[2]; };
__device__ __forceinline__ NtFragAddr nt_frag_addr(const u16* lds_base, int a_elem_off, int b_elem_off, int wm, int wn, int l31, int lh) {
  NtFragAddr f;
  const unsigned base = lds_addr(lds_base);
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int ra = wm * 64 + i * 32 + l31, rb = wn * 64 + i * 32 + l31;
    f.a[i] = base + 2u * (unsigned)a_elem_off + (unsigned)(ra * 128) + 16u * (unsigned)(lh ^ gl_sw<64>(ra));
    f.b[i] = base + 2u * (unsigned)b_elem_off + (unsigned)(rb * 128) + 16u * (unsigned)(lh ^ gl_sw<64>(rb));
  }
  return f;
}
#define NT_DSREAD(dst, addr) asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr))
template <bool SWAP = false>          // SWAP: C^T = B.A^T (lane = row of C, registers = 4 consecutive columns)
__device__ __forceinline__ void nt_compute_step(const NtFragAddr& f, unsigned stage_byte_off, f32x16 (&acc)[2][2]) {
  u32x4v fa[2][2], fb[2][2];          // [parity][i]
  const unsigned a0 = f.a[0] + stage_byte_off, a1 = f.a[1] + stage_byte_off;
  const unsigned b0 = f.b[0] + stage_byte_off, b1 = f.b[1] + stage_byte_off;
#define NT_ISSUE(KS, PAR)                                                                            \
  NT_DSREAD(fa[PAR][0], a0 ^ (32u * (KS))); NT_DSREAD(fb[PAR][0], b0 ^ (32u * (KS)));                \
  NT_DSREAD(fa[PAR][1], a1 ^ (32u * (KS))); NT_DSREAD(fb[PAR][1], b1 ^ (32u * (KS)));
#define NT_MFMA(PAR)                                                                                 \
  _Pragma("unroll") for (int i = 0; i < 2; i++)                                                      \
    _Pragma("unroll") for (int j = 0; j < 2; j++)                                                    \
      acc[i][j] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&fb[PAR][j]), \
                                                                 *reinterpret_cast<const bf16x8*>(&fa[PAR][i]), acc[i][j], 0, 0, 0) \
                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&fa[PAR][i]), \
                                                                 *reinterpret_cast<const bf16x8*>(&fb[PAR][j]), acc[i][j], 0, 0, 0);
  NT_ISSUE(0, 0)
  NT_ISSUE(1, 1)
  asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  NT_MFMA(0)
  __builtin_amdgcn_sched_barrier(0);
  NT_ISSUE(2, 0)
  asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  NT_MFMA(1)
  __builtin_amdgcn_sched_barrier(0);
  NT_ISSUE(3, 1)
  asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  NT_MFMA(0)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  NT_MFMA(1)
#undef NT_ISSUE
#undef NT_MFMA
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient  C[N,K] += A[R,N]^T . B[R,K]
// ---------------------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};

// One operand's share of a stage of the 64-row kernels under the zero-block rule: an image of [64 r][CHUNKS * 8 columns] from
// column col0 of G on, NL loads per wave of a workgroup of NWAVES waves.  The caller issues the loads in its own order.
template <int NL, int CHUNKS, int NWAVES>
struct tn_operand_image {
  const u16* src[NL];
  int row[NL];
  int col_ok[NL];          // (pointers first and the flag an int: as {int, bool, pointer} gemm_tn_256_kernel took two more VGPRs)
  static_assert(CHUNKS == 16 || CHUNKS == 32, "128 or 256 columns");
  __device__ __forceinline__ void set(const u16* __restrict__ G, int col0, int ncols, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NL; i++) {
      const int p = (i * NWAVES + wave) * 64 + lane, r = p >> (CHUNKS == 32 ? 5 : 4), c = (p & (CHUNKS - 1)) ^ ((r & 3) << 2);
      row[i] = r; col_ok[i] = col0 + c * 8 < ncols; src[i] = G + col0 + c * 8;
    }
  }
  // load i of the stage that begins at row r0 of G (row stride ld): into image (the operand's image of that stage)
  __device__ __forceinline__ void load(int i, int r0, int r_end, int64_t ld, u16* image, int wave) const {
    const int r = r0 + row[i];
    lds_dma16((r < r_end && col_ok[i]) ? src[i] + (int64_t)r * ld : reinterpret_cast<const u16*>(g_zero16), image + (i * NWAVES + wave) * 512);
  }
};

// Per-lane byte address for the transposed fragment reads of the 32-column operand block that begins at column col of an image
// at LDS byte address lds0: 16-lane group tg = (lane >> 4) & 1 covers columns 16 tg .. + 15 of the block and k-half lh; lane
// 4 tq + tp of the group supplies LDS row 8 lh + tq (+ 4 for the second read of a k16-step, + 16 per k16-step), columns 4 tp .. + 3.
template <int ROW_ELEMS>
__device__ __forceinline__ unsigned tn_frag_base(unsigned lds0, int col, int lane) {
  const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1, lh = lane >> 5;
  const int c = col + 16 * tg + 4 * tp;
  return lds0 + 2u * (unsigned)((8 * lh + tq) * ROW_ELEMS + (((c >> 3) ^ (tq << 2)) << 3) + (c & 7));
}

#define TR_READ(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
// One 64-row step of a wavefront's 64 x 64 block, the weight gradient's nt_compute_step: 4 k16-steps of 2 x 2 MFMA, the reads
// of k16-step ks + 1 in flight under the MFMAs of ks.  The reads are inline asm with hand-counted lgkmcnt: hipcc otherwise
// orders every ds_read_b64_tr_b16 behind the LDS-DMA of the NEXT stage (s_waitcnt vmcnt(0) at the top of each step), which
// serialises the DMA with the MFMAs.  a0 / a1, b0 / b1: tn_frag_base of the wave's two blocks of each operand plus the stage's
// byte offset.  A's image has A_STEP_BYTES per k16-step (16 rows) and A_HALF_BYTES per 4 rows; B's image is [64][128]: 4096, 1024.
template <int A_STEP_BYTES, int A_HALF_BYTES>
__device__ __forceinline__ void tn_compute_step(unsigned a0, unsigned a1, unsigned b0, unsigned b1, f32x16 (&acc)[2][2]) {
  u32x2v fa[2][2][2], fb[2][2][2];          // [parity][i][t]
#define TN_ISSUE(KS, PAR)                                                                                                \
  TR_READ(fa[PAR][0][0], a0, (KS) * A_STEP_BYTES); TR_READ(fa[PAR][0][1], a0, (KS) * A_STEP_BYTES + A_HALF_BYTES);     \
  TR_READ(fa[PAR][1][0], a1, (KS) * A_STEP_BYTES); TR_READ(fa[PAR][1][1], a1, (KS) * A_STEP_BYTES + A_HALF_BYTES);     \
  TR_READ(fb[PAR][0][0], b0, (KS) * 4096); TR_READ(fb[PAR][0][1], b0, (KS) * 4096 + 1024);                             \
  TR_READ(fb[PAR][1][0], b1, (KS) * 4096); TR_READ(fb[PAR][1][1], b1, (KS) * 4096 + 1024);
#define TN_MFMA(PAR)                                                           \
  {                                                                            \
    bf16x8 af[2], bfr[2];                                                      \
    _Pragma("unroll") for (int i = 0; i < 2; i++) {                            \
      const uint4 ua = make_uint4(fa[PAR][i][0][0], fa[PAR][i][0][1], fa[PAR][i][1][0], fa[PAR][i][1][1]); \
      const uint4 ub = make_uint4(fb[PAR][i][0][0], fb[PAR][i][0][1], fb[PAR][i][1][0], fb[PAR][i][1][1]); \
      af[i] = *reinterpret_cast<const bf16x8*>(&ua);                           \
      bfr[i] = *reinterpret_cast<const bf16x8*>(&ub);                          \
    }                                                                          \
    _Pragma("unroll") for (int i = 0; i < 2; i++)                              \
      _Pragma("unroll") for (int j = 0; j < 2; j++)                            \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0); \
  }
  TN_ISSUE(0, 0)
  TN_ISSUE(1, 1)
  asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  TN_MFMA(0)
  __builtin_amdgcn_sched_barrier(0);
  TN_ISSUE(2, 0)
  asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  TN_MFMA(1)
  __builtin_amdgcn_sched_barrier(0);
  TN_ISSUE(3, 1)
  asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  TN_MFMA(0)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0);
  TN_MFMA(1)
#undef TN_ISSUE
#undef TN_MFMA
}

// A wave's 64 x (32 NJ) block of C[n][k], rows from n_origin and columns from k_origin on: row n in registers, column k on the
// lane -> 128-byte contiguous segments per row.  DET = false adds into the gradient atomically; DET (the deterministic forms):
// C is this row split's slot of the caller's scratch with ldc = K, the partial tile is STORED and det_reduce_kernel
// (elementwise.hip) adds the slots in ascending order.  The row index is acc_row summed left to right, not a call: signed adds
// are not reassociated, and with the call's grouping the grouped 256 x 256 kernel took 15 more VGPRs.
template <bool DET, int NJ>
__device__ __forceinline__ void tn_store_tile(const f32x16 (&acc)[2][NJ], float* __restrict__ C, int64_t ldc, int N, int K, int n_origin,
                                              int k_origin, int lane) {
  const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int k = k_origin + j * 32 + l31;
    if (k >= K) continue;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int n = n_origin + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;          // acc_row, summed left to right
        if constexpr (DET) {
          if (n < N) C[(int64_t)n * ldc + k] = acc[i][j][r];
        } else {
          if (n < N) atomicAdd(C + (int64_t)n * ldc + k, acc[i][j][r]);
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------------------
// The software-pipelined k-step of the two 256 x 256 kernels (gemm_nt_persist256_kernel, tn_256x256_tile): a wave's 64 x 128
// block is 2 x 4 accumulators and a stage holds two k16-steps.  The six fragment reads of a k16-step (two A blocks, four B
// blocks) sit in the gaps between the MFMAs of the k16-step before it, one block per gap and none in a burst; the stage's one
// barrier sits between its two MFMA groups, and MID - the next stage's DMA - runs after the first MFMA of the second group.
// A kernel supplies its own RA(KS, I, SO) / RB(KS, J, SO) (read block I / J of k16-step KS at stage byte offset SO) and
// MM(KS, I, J) (one MFMA), each ending in T256_SB, and keeps its own wait ladder: the reads differ (ds_read_b128 against two
// ds_read_b64_tr_b16), so do the operand order of the MFMA and what vmcnt has to count.
// ---------------------------------------------------------------------------------------------------------
#define T256_SB __builtin_amdgcn_sched_barrier(0);
// the reads of a tile's first k16-step (stage 0, nothing to hide them under)
#define T256_FIRST_READS(RA, RB) RA(0, 0, 0u) RB(0, 0, 0u) RB(0, 1, 0u) RB(0, 2, 0u) RB(0, 3, 0u) RA(0, 1, 0u)
// the MFMAs of k16-step KS with the reads of k16-step KN (at stage offset SO) in their gaps; MID runs after the first MFMA
#define T256_GROUP_READING(RA, RB, MM, KS, KN, SO, MID)                                                                    \
  MM(KS, 0, 0) MID RA(KN, 0, SO) MM(KS, 0, 1) RB(KN, 0, SO) MM(KS, 0, 2) RB(KN, 1, SO) MM(KS, 0, 3) RB(KN, 2, SO)          \
  MM(KS, 1, 0) RB(KN, 3, SO) MM(KS, 1, 1) RA(KN, 1, SO) MM(KS, 1, 2) MM(KS, 1, 3)
// the MFMAs of a tile's last k16-step: nothing left to read
#define T256_GROUP(MM, KS) MM(KS, 0, 0) MM(KS, 0, 1) MM(KS, 0, 2) MM(KS, 0, 3) MM(KS, 1, 0) MM(KS, 1, 1) MM(KS, 1, 2) MM(KS, 1, 3)
