// The tile walk the attention kernels share (attention_fwd.hip, attention_bwd2.hip, attention_fp8.hip, attention_readout.hip):
// tile constants, the K image, the workgroup decode, and the contract of the tile lists - what a q_kt entry, a key-tile flag
// and slot 15 of the mask product mean.  Device code only; every function is inlined into a kernel's prologue (or, for the
// mask operand, its masked-tile branch), and none of it may move a kernel's MFMA loop: tools/isa_diff.py against the parent
// commit is the check (profiles/attention_common_isa.md).  attention_bwd1.hip has another workgroup and a generated
// schedule: it does not use this header.
#pragma once
#include "common.h"

#define AQ 128      // query rows per workgroup (query-tile-major kernels)
#define AK 64       // keys per tile
#define DH 64       // head dim (fixed)
#define MAX_KTILES 512
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

// K tile image: [64 keys][64 d] bf16, 128-byte rows, chunk c (16 B) of row r at c ^ ((r>>1)&7): row reads (ds_read_b128) only.
// k_swz: the element offset of the chunk inside its row (the LDS-DMA kernels, which write lane-linear, apply it to the SOURCE
// column); k_off: the element offset inside the image
__device__ __forceinline__ int k_swz(int r, int c) { return (c ^ ((r >> 1) & 7)) << 3; }
__device__ __forceinline__ int k_off(int r, int c) { return r * 64 + k_swz(r, c); }

// ---- workgroup decode, query-tile-major: grid (query tiles, heads, samples).  XCD-aware order: the query tiles of one
// (sample, head) read the same K / V, so they are given to one XCD (in launch order they were dealt round all eight and every
// L2 fetched every K / V: 1,128 MB per launch against 250 MB).  dbg = knob 9; bit 16: launch order (A/B).  lin0 is the
// launch-order id (the trace builds pick their wavefront by it).
struct attn_wg { int lin0, qt, h, b; };
__device__ __forceinline__ attn_wg attn_wg_decode(const int32_t* q_order, int dbg) {
  const int lin0 = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
  const int lin = (dbg & 16) ? lin0 : xcd_remap(lin0, (int)(gridDim.x * gridDim.y * gridDim.z));
  return {lin0, q_order[lin % (int)gridDim.x], (lin / (int)gridDim.x) % (int)gridDim.y, lin / (int)(gridDim.x * gridDim.y)};
}
// ---- the same for the key-block-major dK / dV kernels: grid (key blocks, heads, samples), k_wg = per launch slot the four
// int32 {key block, begin of its list in k_qt, length of the list, first query tile of the list}
struct attn_kwg { int kbi, it_begin, n_it, first_qt, h, b; };
__device__ __forceinline__ attn_kwg attn_kwg_decode(const int32_t* k_wg, int dbg) {
  const int lin0 = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
  const int lin = (dbg & 16) ? lin0 : xcd_remap(lin0, (int)(gridDim.x * gridDim.y * gridDim.z));
  const int4 w = reinterpret_cast<const int4*>(k_wg)[lin % (int)gridDim.x];
  return {w.x, w.y, w.z, w.w, (lin / (int)gridDim.x) % (int)gridDim.y, lin / (int)(gridDim.x * gridDim.y)};
}
// does key block kbi (BKEYS keys) hold a valid key in this sample?  (flags_g: the sample's key-tile flags)
template <int BKEYS>
__device__ __forceinline__ bool attn_kblock_live(const uint8_t* flags_g, int n_ktiles, int kbi) {
  int live = 0;
  for (int t = 0; t < BKEYS / AK; t++) { const int kt = kbi * (BKEYS / AK) + t; if (kt < n_ktiles) live |= flags_g[kt]; }
  return live != 0;
}

// this lane's query row: row arow of query tile qt (wavefront w owns rows 32 w .. + 31, lane l and lane l + 32 share row l & 31).
// Rows past nq are clamped to the last row (they load valid memory and compute, qvalid keeps them from storing).
__device__ __forceinline__ int attn_qrow(int qt, int arow, int nq, bool& qvalid) {
  int qrow = qt * AQ + arow;
  qvalid = qrow < nq;
  if (qrow > nq - 1) qrow = nq - 1;
  return qrow;
}

// Q fragments, the B operand of S^T = K Q^T held for the whole kernel: the lane holds Q[q][16 s + 8 lh + j] of its row
// (qp: the row, this head)
__device__ __forceinline__ void attn_load_qf(bf16x8 (&qf)[4], const u16* qp, int lh) {
#pragma unroll
  for (int s = 0; s < 4; s++) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 8 * lh + 16 * s);
}

// ---- a sample's key-tile flags (mca_build_keyinfo: 0 no valid key in the 64-key tile, 1 mixed, 2 all valid) into LDS, by a
// workgroup of 256 threads; the caller's barrier makes them visible
__device__ __forceinline__ void attn_stage_flags(uint8_t* flags_s, const uint8_t* flags_g, int n, int tid) {
  for (int i = tid; i < n; i += 256) flags_s[i] = flags_g[i];
}

// ---- the tile list of query tile qt, minus the tiles whose keys are all padded in this sample; wavefront 0 calls it, between
// two barriers.  Compacted ONCE: reading the CSR entry and the flag of the NEXT live tile at the top of every iteration was a
// chain of a scalar global load and an LDS read in front of the K / V loads (most of the 1,500 cycles the traced "S" phase
// of attn_fwd_kernel took).
// Entry format, q_kt[q_ptr[qt] .. q_ptr[qt + 1]) in and live_s[0 .. n) out:
//   bits 0..30  the 64-key tile
//   bit 31 in   the tile is structurally FULL for this query tile: every (query, key group) pair of it is allowed
//   bit 31 out  FOLD = false: unchanged (the kernel still asks flags_s[tile] != 2 per tile);
//               FOLD = true: no mask is needed for this sample - structurally full AND flag 2, every key of the tile valid
// Returns n, which is also left in *n_live_s.
template <bool FOLD>
__device__ __forceinline__ int attn_compact_tiles(const int32_t* q_ptr, const uint32_t* q_kt, int qt, const uint8_t* flags_s,
                                                  uint32_t* live_s, int* n_live_s, int lane) {
  const int lb = q_ptr[qt], le = q_ptr[qt + 1];
  int n = 0;
  for (int i0 = lb; i0 < le; i0 += 64) {
    const int i = i0 + lane;
    const uint32_t e = i < le ? q_kt[i] : 0u;
    const uint8_t fl = i < le ? flags_s[e & 0x7fffffffu] : (uint8_t)0;
    const bool keep = fl != 0;
    const unsigned long long m = __ballot(keep);
    if (keep) live_s[n + __popcll(m & ((1ull << lane) - 1ull))] = FOLD ? (e & 0x7fffffffu) | ((e >> 31) && fl == 2 ? 0x80000000u : 0u) : e;
    n += __popcll(m);
  }
  if (lane == 0) *n_live_s = n;
  return n;
}

// ---- the query side of the mask as a matrix product (mca_build_keyhot): Qblk[q][g] = group g visible to the query ? 0 :
// -32768 (bf16 0xC700), against the one-hot key groups of the tile.  Slot 15 collects the padded keys and the keys past nk
// and is ALWAYS blocked.  Lane half lh holds groups 8 lh .. 8 lh + 7 of its query.
// attn_qm8: the visible-bits of those eight groups, slot 15 never; attn_qblk8: the operand from them (cheap enough to rebuild
// per masked tile where four more registers held for the whole kernel would spill); attn_qblk: the operand from the query's
// mask word.
__device__ __forceinline__ uint32_t attn_qm8(uint32_t qm, int lh) { return ((qm >> (8 * lh)) & 0xffu) & (lh ? 0x7fu : 0xffu); }
__device__ __forceinline__ bf16x8 attn_qblk8(uint32_t qm8) {
  u32x4v qb;
#pragma unroll
  for (int w = 0; w < 4; w++)
    qb[w] = (((qm8 >> (2 * w)) & 1u) ? 0u : 0xC700u) | (((qm8 >> (2 * w + 1)) & 1u) ? 0u : 0xC7000000u);
  return *reinterpret_cast<const bf16x8*>(&qb);
}
__device__ __forceinline__ bf16x8 attn_qblk(uint32_t qm, int lh) {
  bf16x8 qblk;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int g = 8 * lh + j;
    qblk[j] = (g < 15 && ((qm >> g) & 1u)) ? (short)0 : (short)0xC700;
  }
  return qblk;
}

// ---- forward epilogue: op = the lane's row of o (this head) = O^T / l - or, on a uniform row, the mean of V (vm: this (sample,
// head) of vmean).  The lane holds elements 32 n + 8 g + 4 lh .. + 3 of the row in accumulator n, registers 4 g .. 4 g + 3.
// (The dQ and dK / dV stores stay in their kernels: shared, they moved those kernels' loops.)
__device__ __forceinline__ void attn_store_o(u16* op, const float* vm, const f32x16 (&o)[2], float inv, bool uniform, int lh) {
#pragma unroll
  for (int n = 0; n < 2; n++)
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int d = n * 32 + 8 * g + 4 * lh;
      float v0, v1, v2, v3;
      if (uniform) { v0 = vm[d]; v1 = vm[d + 1]; v2 = vm[d + 2]; v3 = vm[d + 3]; }
      else { v0 = o[n][4 * g] * inv; v1 = o[n][4 * g + 1] * inv; v2 = o[n][4 * g + 2] * inv; v3 = o[n][4 * g + 3] * inv; }
      uint2 pk; pk.x = pack2bf(v0, v1); pk.y = pack2bf(v2, v3);
      *reinterpret_cast<uint2*>(op + d) = pk;
    }
}
