// bf16 MFMA GEMMs for every Linear of the MCA step (forward, data-gradient and weight-gradient).
//
//   mca_gemm_nt     C[M,N]  = A[M,K] · B[N,K]^T      both operands K-contiguous (Linear forward with
//                                                     x[M,K], W[N,K]; data-gradient with the transposed
//                                                     bf16 weight copy)
//   mca_gemm_nt_lnres / _geglu_fwd / _geglu_bwd       the same GEMM with a fused epilogue (residual LayerNorm
//                                                     recomputed; FF1 + GEGLU; W2 data gradient + GEGLU')
//   mca_gemm_nt_geglu_fwd_saved / _bwd_saved          the two GEGLU fusions with the backward's factors [gelu(gate) | a gelu'(gate)]
//                                                     kept in h's place: the backward epilogue only multiplies
//   mca_gemm_nt_res_lnbwd                             the same GEMM (N = 512) owning whole rows of C, the trunk LayerNorm backward of
//                                                     dy = C (+ residual) in its epilogue: dy is never stored
//   mca_gemm_tn_acc C[N,K] += A[R,N]^T · B[R,K]      both operands reduction-major (weight gradient:
//                                                     dW = dY^T · X), operands fetched from LDS with the
//                                                     gfx950 transposed read ds_read_b64_tr_b16
//
// Kernels (all v_mfma_f32_32x32x16_bf16, operands global -> LDS by global_load_lds_dwordx4 with the XOR swizzle
// applied to the source address and again on the fragment reads, counted s_waitcnt vmcnt so the DMA stays in flight
// across the raw s_barrier of a k-step):
//   gemm_nt_persist_kernel   256x128 tiles walked by one workgroup per CU; next tile's DMA under a wave-private,
//                            all-asm epilogue; bf16 / plain fp32 outputs and the two GEGLU fusions (M >= 2048)
//   gemm_nt_256_kernel       256x128x64, three stages, one tile per workgroup; fp32 + residual outputs (residual tile
//                            prefetched into registers; optional LayerNorm recompute), fallback for odd shapes
//   gemm_nt_glds_kernel      128x128x64, two stages: small M
//   gemm_nt_rows_kernel      128x512x32, three stages, one tile of whole rows per workgroup; LayerNorm-backward epilogue
//   gemm_tn_256x256_kernel / gemm_tn_256_kernel / gemm_tn_kernel   weight gradient, split over rows + fp32 atomics
// Workgroup ids are remapped (xcd_remap) so that workgroups sharing operands sit on one XCD / L2.
#include "common.h"
#include "gemm_plan.h"          // tile geometry, LDS sizes and the dispatch rules (plain host C++)
#include "gemm_tile.h"          // the device code the kernels share: operand images, staging, fragments, k-steps, stores
#include "ln_rows.h"            // the trunk LayerNorm backward's row body (the full-row kernel's epilogue)

static int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}

// Persistent kernel: tile index -> (row tile tm, column tile tn).  Row tiles are taken in groups of PS_PANELS: index =
// (group, tn, tm in group), so the 32 workgroups of an XCD (contiguous indices, xcd_remap) work on PS_PANELS activation
// panels x 8 weight tiles at a time (1 MiB + 1 MiB of the 4 MiB L2) and a panel group stays resident while the column
// tiles sweep past it; in row-major tile order all 22 column tiles of FF1 (2.9 MiB of weights) are live at once and the
// activation panels are re-fetched 9 times (PMC FETCH_SIZE x 2: 756 MB per launch against 86 MB of operands; 436 MB
// with the groups; step -0.36 ms in-process; 4, 8 and 16 panels per group measure the same, 2 is worse).
#define PS_PANELS 4
__device__ __forceinline__ void ps_tile_decode(int tile, int tiles_m, int tiles_n, int flat, int& tm, int& tn) {
  if (flat == 1) { tm = tile / tiles_n; tn = tile % tiles_n; return; }
  const int P = flat > 1 ? flat : PS_PANELS;
  const int per_group = P * tiles_n;
  const int g = tile / per_group;
  const int gh = (g + 1) * P <= tiles_m ? P : tiles_m - g * P;          // panels in this (last) group
  const int rem = tile - g * per_group;
  tn = rem / gh; tm = g * P + rem % gh;
}

// Fused GEGLU backward (model.py:35-38 autograd) for 8 consecutive columns n..n+7 of row m of dg = dY·W2 (fp32 in v):
// h = [a | gate] (bf16, row stride ldh, halves ip apart);  dh_a = dg*gelu(gate),  dh_gate = dg*a*gelu'(gate).
// SAVED: h holds the saved factors s = [gelu(gate) | a*gelu'(gate)] of the forward (mca_gemm_nt_geglu_fwd_saved) instead:
// dh_a = dg*s_lo, dh_gate = dg*s_hi.
template <bool SAVED>
__device__ __forceinline__ void geglu_bwd_piece(const float (&v)[8], const u16* __restrict__ h, u16* __restrict__ dh, int64_t ldh,
                                                int ip, int64_t m, int n) {
  const bf16x8 av = *reinterpret_cast<const bf16x8*>(h + m * ldh + n);
  const bf16x8 gv = *reinterpret_cast<const bf16x8*>(h + m * ldh + ip + n);
  bf16x8 da, dgt;
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const float g = bf2f((u16)gv[e]), a = bf2f((u16)av[e]);
    if (SAVED) {
      da[e] = (short)f2bf(v[e] * a);
      dgt[e] = (short)f2bf(v[e] * g);
      continue;
    }
    float ge, dge;
    gelu_pair(g, ge, dge);
    da[e] = (short)f2bf(v[e] * ge);
    dgt[e] = (short)f2bf(v[e] * a * dge);
  }
  *reinterpret_cast<bf16x8*>(dh + m * ldh + n) = da;
  *reinterpret_cast<bf16x8*>(dh + m * ldh + ip + n) = dgt;
}

// Epilogue through LDS (the kernels with k-steps of 64: the 64 KiB of operand buffers hold exactly one 128x128 fp32 tile).  The
// accumulators are written lane = column / register = row, then every thread reads whole 16-byte pieces of rows,
// adds bias / residual with 16-byte loads and stores 16 bytes: 4x (fp32) or 8x (bf16) fewer store instructions,
// every global access a full 128-byte-line segment of a row.
// Second half of the LDS epilogue: the fp32 C tile (ROWS x 128, row-major in cs) leaves as whole 16-byte row pieces, bias /
// residual / GEGLU-backward fused; THREADS threads, every global access a full 128-byte-line segment of a row.
template <bool OUT_BF16, int RES, int EPI, int ROWS, int THREADS>
__device__ __forceinline__ void nt_epilogue_rows(const float* __restrict__ cs, void* __restrict__ Cv, int64_t ldc,
                                                 const float* __restrict__ bias, const float* __restrict__ residual,
                                                 int64_t ldres, int64_t res_period, int M, int N, int m0, int n0, int tid) {
  constexpr int EPT = OUT_BF16 ? 8 : 4;          // elements per thread per piece
  constexpr int PPR = 128 / EPT;                 // pieces per row
#pragma unroll 4
  for (int it = 0; it < (ROWS * PPR) / THREADS; it++) {
    const int id = tid + THREADS * it;
    const int row = id / PPR, c0 = (id % PPR) * EPT;
    const int m = m0 + row, n = n0 + c0;
    if (m >= M || n >= N) continue;
    float v[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(cs + row * 128 + c0 + e);
      v[e] = t[0]; v[e + 1] = t[1]; v[e + 2] = t[2]; v[e + 3] = t[3];
    }
    const bool full = n + EPT <= N;
    if (EPI == 1 || EPI == 3) {          // GEGLU backward: Cv = dh, residual = h (EPI 3: the saved factors s), bf16, ldres = row stride of both, N = ip (multiple of 8)
      if (OUT_BF16) geglu_bwd_piece<EPI == 3>(reinterpret_cast<const float(&)[8]>(v), reinterpret_cast<const u16*>(residual),
                                              reinterpret_cast<u16*>(Cv), ldres, N, (int64_t)m, n);
      continue;
    }
    if (bias) {
#pragma unroll
      for (int e = 0; e < EPT; e++) if (full || n + e < N) v[e] += bias[n + e];
    }
    if (RES != 0) {
      const int64_t rr = RES == 2 ? (int64_t)(m % (int)res_period) : (int64_t)m;
      const float* rp = residual + rr * ldres + n;
      if (full && (((uintptr_t)rp) & 15) == 0) {
#pragma unroll
        for (int e = 0; e < EPT; e += 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(rp + e);
          v[e] += t[0]; v[e + 1] += t[1]; v[e + 2] += t[2]; v[e + 3] += t[3];
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPT; e++) if (n + e < N) v[e] += rp[e];
      }
    }
    if (OUT_BF16) {
      u16* cp = reinterpret_cast<u16*>(Cv) + (int64_t)m * ldc + n;
      if (full && (((uintptr_t)cp) & 15) == 0) {
        uint4 pk;
        pk.x = pack2bf(v[0], v[1]); pk.y = pack2bf(v[2], v[3]); pk.z = pack2bf(v[4 % EPT], v[5 % EPT]); pk.w = pack2bf(v[6 % EPT], v[7 % EPT]);
        *reinterpret_cast<uint4*>(cp) = pk;
      } else {
#pragma unroll
        for (int e = 0; e < EPT; e++) if (n + e < N) cp[e] = f2bf(v[e]);
      }
    } else {
      float* cp = reinterpret_cast<float*>(Cv) + (int64_t)m * ldc + n;
      if (full && (((uintptr_t)cp) & 15) == 0) {
        *reinterpret_cast<f32x4*>(cp) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int e = 0; e < EPT; e++) if (n + e < N) cp[e] = v[e];
      }
    }
  }
}

template <bool OUT_BF16, int RES, int EPI>
__device__ __forceinline__ void nt_epilogue_lds(f32x16 (&acc)[2][2], float* __restrict__ cs, void* __restrict__ Cv, int64_t ldc,
                                                const float* __restrict__ bias, const float* __restrict__ residual,
                                                int64_t ldres, int64_t res_period, int M, int N, int m0, int n0, int wm, int wn,
                                                int l31, int lh, int tid) {
  acc_to_lds_tile(acc, cs, wm, wn, l31, lh);
  __syncthreads();
  nt_epilogue_rows<OUT_BF16, RES, EPI, 128, 256>(cs, Cv, ldc, bias, residual, ldres, res_period, M, N, m0, n0, tid);
}

// ---------------------------------------------------------------------------------------------------------
// NT kernel with direct global->LDS staging (global_load_lds_dwordx4): no staging VGPRs, no ds_write pass.
// The LDS destination of one wave-instruction is linear (wave base + lane*16 B), so the XOR swizzle is applied
// to the per-lane SOURCE address and again on the fragment reads (cdna guide, rule 21; the image and its swizzle: gemm_tile.h,
// where the fragment addresses and the k-step nt_compute_step live too).
// ---------------------------------------------------------------------------------------------------------
template <bool OUT_BF16, int RES, int BKT, int EPI>
__global__ __launch_bounds__(256) void gemm_nt_glds_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, void* __restrict__ Cv,
    int64_t ldc, const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldres,
    int64_t res_period, int M, int N, int K, int tiles_n, int nwg) {
  constexpr int CH = BKT / 8;                 // 16-byte chunks per tile row
  constexpr int TILE = 128 * BKT;             // elements per operand tile
  constexpr int NI = CH / 2;                  // wave-instructions per operand tile per wave
  __shared__ __attribute__((aligned(16))) u16 lds[4 * TILE];
  u16* As = lds;
  u16* Bs = lds + 2 * TILE;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  const u16* ga[NI];
  const u16* gb[NI];
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int p = (i * 4 + wave) * 64 + lane;           // linear chunk position inside the tile image
    const int r = p / CH, cp = p % CH;
    const int c = cp ^ gl_sw<BKT>(r);                   // logical chunk stored at this position
    int ra = m0 + r; if (ra > M - 1) ra = M - 1;
    int rb = n0 + r; if (rb > N - 1) rb = N - 1;
    ga[i] = A + (int64_t)ra * lda + c * 8;
    gb[i] = B + (int64_t)rb * ldb + c * 8;
  }
  auto stage = [&](int k0, int buf) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      lds_dma16(ga[i] + k0, As + buf * TILE + (i * 4 + wave) * 512);
      lds_dma16(gb[i] + k0, Bs + buf * TILE + (i * 4 + wave) * 512);
    }
  };
  f32x16 acc[2][2];
  acc_clear(acc);

  const int nkt = K / BKT;
  const NtFragAddr frag = nt_frag_addr(lds, 0, 2 * TILE, wm, wn, l31, lh);
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nkt; kt++) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) stage((kt + 1) * BKT, cur ^ 1);
    nt_compute_step(frag, (unsigned)cur * (unsigned)(TILE * 2), acc);
    __syncthreads();          // waits for this wave's LDS-DMA (vmcnt(0)) and for every wave's reads of `cur`
  }
  static_assert(BKT == 64, "the LDS epilogue needs the 64 KiB of operand buffers");
  nt_epilogue_lds<OUT_BF16, RES, EPI>(acc, reinterpret_cast<float*>(lds), Cv, ldc, bias, residual, ldres, res_period, M, N, m0, n0,
                                 wm, wn, l31, lh, tid);
}

// ---------------------------------------------------------------------------------------------------------
// NT kernel, large-M variant: 256x128x64 tile, 8 wavefronts (4x2, 64x64 each), THREE LDS stages (144 KiB) filled
// by global_load_lds two k-steps ahead; one raw s_barrier per k-step with a counted s_waitcnt vmcnt so the DMA of
// the next stage stays in flight across the barrier (cdna guide: "Pipelining across barriers").  25 % fewer
// global->LDS bytes per flop than the 128x128 tile.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wait_vmcnt(int n) {          // s_waitcnt needs an immediate
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
  }
}
// PF = 1 (fp32 output with a full-row residual, whole column tile inside N): the residual tile (256x128 fp32 =
// 16 float4 per thread) is fetched into registers two pieces per k-step during the first 8 k-steps, so the epilogue
// does not start with a 128 KiB read.  vmcnt counts DMA and residual loads together, in issue order: the wait in
// front of step kt lets everything issued after stage kt's DMA stay in flight.
// EPI = 2 (with PF = 1): the residual is LayerNorm(x) RECOMPUTED from the layer's saved pre-norm tensor x (= `residual`)
// and its row statistics: (x - ln_mean[m]) * ln_rstd[m] * ln_gamma[n] — the normed fp32 tensor is then never written
// by the LayerNorm kernel nor read here (same bytes read, 166 MB less written per LayerNorm at b = 32).  The 256 rows'
// statistics wait in 2 KiB of LDS behind the three stages.
template <bool OUT_BF16, int RES, int PF, int EPI>
__global__ __launch_bounds__(512) void gemm_nt_256_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, void* __restrict__ Cv,
    int64_t ldc, const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldres,
    int64_t res_period, int M, int N, int K, int tiles_n, int nwg, const float* __restrict__ ln_mean = nullptr,
    const float* __restrict__ ln_rstd = nullptr, const float* __restrict__ ln_gamma = nullptr) {
  extern __shared__ __attribute__((aligned(16))) u16 lds2[];
  constexpr int STAGE = nt256_image::STAGE;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tm = tile / tiles_n, tn = tile % tiles_n;
  const int m0 = tm * BM2, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  nt256_image img{wave, lane};
  img.set_tile(A, lda, B, ldb, M, m0, [&](int r) { int rb = n0 + r; if (rb > N - 1) rb = N - 1; return rb; });
  f32x16 acc[2][2];
  acc_clear(acc);

  const int nkt = K / 64;
  const NtFragAddr frag = nt_frag_addr(lds2, 0, BM2 * 64, wm, wn, l31, lh);
  f32x4 rres[PF ? 16 : 1];
  auto res_issue = [&](int it) -> f32x4 {          // piece `it` of this thread's share of the residual tile
    const int id = tid + 512 * it, row = id >> 5, c0 = (id & 31) * 4;
    // rows past M are CLAMPED, not skipped: the counted vmcnt waits below assume that every wave issues every one of
    // these loads (a tile crossing M used to skip them and then waited for too few of its DMA loads: a rare stale-LDS
    // race in the last 64 rows of the out-proj / FF2 / data-gradient GEMMs, caught by the bit-exactness test)
    int m = m0 + row; if (m > M - 1) m = M - 1;
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(residual + (int64_t)m * ldres + n0 + c0));          // streamed once
  };
  float* lnstat = reinterpret_cast<float*>(lds2 + 3 * STAGE);          // EPI == 2: [256] mean, [256] rstd
  float ln_val = 0.f;
  if (EPI == 2) {          // issued before the DMA so that its (compiler-counted) wait leaves the DMA in flight
    int m = m0 + (tid & 255); if (m > M - 1) m = M - 1;
    ln_val = tid < 256 ? ln_mean[m] : ln_rstd[m];
  }
  img.stage(lds2, 0, 0);
  if (nkt > 1) img.stage(lds2, 64, 1);
  if (EPI == 2) lnstat[tid] = ln_val;          // visible to every wave after the k-loop's barriers
  int st = 0;
#define NT256_STEP(KT, WAITN)                                                                  \
  {                                                                                            \
    wait_vmcnt(WAITN);                                                                         \
    __builtin_amdgcn_s_barrier();                                                              \
    if ((KT) + 2 < nkt) { int s2 = st + 2; if (s2 >= 3) s2 -= 3; img.stage(lds2, ((KT) + 2) * 64, s2); } \
    nt_compute_step(frag, (unsigned)st * (unsigned)(STAGE * 2), acc);                          \
    st = st == 2 ? 0 : st + 1;                                                                 \
  }
  if (PF) {
    // nkt >= 8 is guaranteed by the host for PF kernels
    NT256_STEP(0, 6)   rres[0] = res_issue(0);   rres[1 % (PF ? 16 : 1)] = res_issue(1);
    NT256_STEP(1, 8)   rres[2 % (PF ? 16 : 1)] = res_issue(2);   rres[3 % (PF ? 16 : 1)] = res_issue(3);
    NT256_STEP(2, 10)  rres[4 % (PF ? 16 : 1)] = res_issue(4);   rres[5 % (PF ? 16 : 1)] = res_issue(5);
    NT256_STEP(3, 10)  rres[6 % (PF ? 16 : 1)] = res_issue(6);   rres[7 % (PF ? 16 : 1)] = res_issue(7);
    NT256_STEP(4, 10)  rres[8 % (PF ? 16 : 1)] = res_issue(8);   rres[9 % (PF ? 16 : 1)] = res_issue(9);
    NT256_STEP(5, 10)  rres[10 % (PF ? 16 : 1)] = res_issue(10); rres[11 % (PF ? 16 : 1)] = res_issue(11);
    NT256_STEP(6, 10)  rres[12 % (PF ? 16 : 1)] = res_issue(12); rres[13 % (PF ? 16 : 1)] = res_issue(13);
    NT256_STEP(7, nkt > 8 ? 10 : 4) rres[14 % (PF ? 16 : 1)] = res_issue(14); rres[15 % (PF ? 16 : 1)] = res_issue(15);
    for (int kt = 8; kt < nkt; kt++) {
      const int more = kt + 1 < nkt ? 6 : 0;
      NT256_STEP(kt, kt == 8 ? 4 + more : (kt == 9 ? 2 + more : more))
    }
  } else {
    for (int kt = 0; kt < nkt; kt++) {
      // this wave's DMA for stage kt has landed once at most the 6 loads of stage kt+1 are outstanding
      NT256_STEP(kt, kt + 1 < nkt ? 6 : 0)
    }
  }
#undef NT256_STEP
  __syncthreads();
  // epilogue through LDS: 256x128 fp32 = 128 KiB
  float* cs = reinterpret_cast<float*>(lds2);
  acc_to_lds_tile(acc, cs, wm, wn, l31, lh);
  __syncthreads();
  if (PF) {
    // fast epilogue: residual already in registers, whole 128-column tile valid, 16-byte stores
    float lnstat_r[PF ? 16 : 1][2];
    f32x4 lng = f32x4{1.f, 1.f, 1.f, 1.f};
    if (EPI == 2) {
      lng = *reinterpret_cast<const f32x4*>(ln_gamma + n0 + (tid & 31) * 4);
#pragma unroll
      for (int it = 0; it < 16; it++) {
        const int row = (tid + 512 * it) >> 5;
        lnstat_r[it % (PF ? 16 : 1)][0] = lnstat[row]; lnstat_r[it % (PF ? 16 : 1)][1] = lnstat[256 + row];
      }
    }
#pragma unroll
    for (int it = 0; it < 16; it++) {
      const int id = tid + 512 * it, row = id >> 5, c0 = (id & 31) * 4;
      const int m = m0 + row;
      if (m < M) {
        f32x4 v = *reinterpret_cast<const f32x4*>(cs + row * 128 + c0);
        f32x4 r = rres[it % (PF ? 16 : 1)];
        if (EPI == 2) {
          const float mu = lnstat_r[it % (PF ? 16 : 1)][0], rs = lnstat_r[it % (PF ? 16 : 1)][1];
#pragma unroll
          for (int e = 0; e < 4; e++) r[e] = (r[e] - mu) * rs * lng[e];
        }
        v[0] += r[0]; v[1] += r[1]; v[2] += r[2]; v[3] += r[3];
        if (bias) { v[0] += bias[n0 + c0]; v[1] += bias[n0 + c0 + 1]; v[2] += bias[n0 + c0 + 2]; v[3] += bias[n0 + c0 + 3]; }
        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(reinterpret_cast<float*>(Cv) + (int64_t)m * ldc + n0 + c0));
      }
    }
    return;
  }
  nt_epilogue_rows<OUT_BF16, RES, EPI, BM2, 512>(cs, Cv, ldc, bias, residual, ldres, res_period, M, N, m0, n0, tid);
}

// ---------------------------------------------------------------------------------------------------------
// PERSISTENT NT kernel (large M, N % 128 == 0): one 512-thread workgroup per CU walks 256x128 tiles.
// Why: with K = 512 a tile is only 8 k-steps; in the one-tile-per-workgroup kernels every CU loads, computes and
// stores in step with all the others, so HBM idles while the matrix pipes run and vice versa, and each tile pays
// its first-load latency and the drain of its stores (a k-loop-less build of the QKV GEMM still took 108 of its 224 us).  Here
//   * the global->LDS DMA of the NEXT tile's first two k-steps is issued before the epilogue of the current one
//     (into stage slots 0 and 1),
//   * the epilogue is wave-private (no workgroup barrier): each wave moves its 64x64 block through an 8 KiB scratch
//     area (the free third stage slot + 16 KiB: 160 KiB of LDS in all) and leaves as whole 128-byte row segments;
//     its global stores drain while the next tile's k-loop runs.
// The MFMA operands are swapped (C^T = B.A^T) so that a lane holds 4 CONSECUTIVE columns of one row: the
// accumulators go to the scratch area as 8/16-byte pieces instead of single elements.
// All epilogue memory instructions are inline asm: (1) hipcc would put s_waitcnt vmcnt(0) in front of its own LDS
// reads while an LDS-DMA is in flight, (2) the counted vmcnt waits of the next k-loop need the exact number of
// younger stores (CDNA4: loads, stores and LDS-DMA retire in issue order).
// vmcnt bookkeeping per wave and tile, in issue order: ... [DMA of the last k-step: 6] [NLD residual / h / bias loads]
// (k-loop goes on: the last two steps wait vmcnt(6 + NLD) and vmcnt(NLD)) [DMA next tile k-step 0: 6] [DMA k-step 1: 6]
// [NST stores]; k-step 0 of the next tile waits vmcnt(6 + NST), k-step 1 vmcnt(NST + 6) (the DMA of k-step 2 is issued
// in between), later steps vmcnt(6).  Tiles that cross M (predicated stores: unknown count) drain with vmcnt(0).
// ---------------------------------------------------------------------------------------------------------
// The epilogue traffic (C tiles, the h / dh tiles of the GEGLU forms: 0.5-0.9 GB per launch) is streamed with the
// non-temporal hint so that it does not evict the activation panels and weight tiles the k-loops re-read from L2
// (GEGLU backward fetched 778 MB against 540 MB of operands; step -0.28 ms in an alternating-process A/B).
#define PS_NT " nt"
#define PS_GLOAD(dst, ptr) asm volatile("global_load_dwordx4 %0, %1, off" PS_NT : "=&v"(dst) : "v"(ptr) : "memory")
// s_nop: a VMEM store of more than 64 bits needs a wait state before a VALU may overwrite its data VGPRs; hipcc
// inserts it for its own stores but cannot see into inline asm
#define PS_GSTORE(ptr, val) asm volatile("global_store_dwordx4 %0, %1, off" PS_NT "\n\ts_nop 1" ::"v"(ptr), "v"(val) : "memory")
#define PS_DSW128(addr, val) asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(val) : "memory")
#define PS_DSW64(addr, val) asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(val) : "memory")
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
template <int N> __device__ __forceinline__ void ps_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// timeline probe (TRACE build only: mca-paper_amd/build.py --trace; knob 0 = 8): workgroup 0 / wave 0 writes s_memtime stamps,
// read back by tools/trace_persist.py; the product build carries neither the stamps nor the clock probe of the grouped kernel
MCA_TRACE_BUFFER(gemm)
#ifdef MCA_TRACE_BUILD
#define PS_STAMP() do { if (tracing && ti < 1024) mca_trace_gemm[ti++] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PS_STAMP() do { } while (0)
#endif

// MODE 0: bf16 out;  1: fp32 out;  2: fp32 out + full-row fp32 residual;  3: fused GEGLU backward (bf16 out, see
// mca_gemm_nt_geglu_bwd: C = dh, residual = h, ldres = row stride of both, N = ip);  4: fused GEGLU forward (see
// mca_gemm_nt_geglu_fwd: B = W1 [2*ip, K], a column tile = 64 "a" rows + the 64 "gate" rows of the same columns,
// C = h [M, 2*ip] bf16, residual = g [M, ip] bf16 with row stride ldres, N = ip, tiles_n = ip / 64);  5 and 6: modes 3 and 4 with
// the saved factors s = [gelu(gate) | a * gelu'(gate)] in the place of h (mca_gemm_nt_geglu_bwd_saved / _fwd_saved): the same
// loads and stores per tile, so NST / NLD / NPRE and every counted wait are those of modes 3 and 4
template <int MODE, bool BIAS>
__global__ __launch_bounds__(512) void gemm_nt_persist_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, void* __restrict__ Cv,
    int64_t ldc, const float* __restrict__ bias, const float* __restrict__ residual, int64_t ldres,
    int M, int N, int K, int tiles_n, int nwg, int dbg) {
  extern __shared__ __attribute__((aligned(16))) u16 lds2[];
  constexpr int STAGE = nt256_image::STAGE;
  constexpr bool BWD = MODE == 3 || MODE == 5, FWD = MODE == 4 || MODE == 6, SAVED = MODE >= 5;
  constexpr int NST = MODE == 0 ? 8 : (FWD ? 12 : 16);         // global stores per wave and tile
  constexpr int NPRE = (MODE == 2 || BWD) ? 16 : 1;
  constexpr int NLD = ((MODE == 2 || BWD) ? 16 : 0) + (BIAS ? (MODE == 0 ? 2 : 1) : 0);          // epilogue input loads per wave and tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int nkt = K / 64;
  const NtFragAddr frag = nt_frag_addr(lds2, 0, BM2 * 64, wm, wn, l31, lh);
  const unsigned lds_base = lds_addr(lds2);
  const unsigned scratch = lds_base + 2u * (unsigned)(STAGE * 2) + (unsigned)wave * 8192u;   // stage slot 2 and the 16 KiB after it

  nt256_image img{wave, lane};
  const int tiles_m = nwg / tiles_n;
  const int flat_order = (dbg >> 5) & 31;          // knob 0 = 32: row-major tile order; 32*P: P panels per group (A/B)
  auto tile_ptrs = [&](int tile) {
    int tm, tn;
    ps_tile_decode(tile, tiles_m, tiles_n, flat_order, tm, tn);
    const int n0 = tn * BN;
    // N % 128 == 0 (MODE 4: N % 64 == 0): no clamp.  MODE 4: tile rows 0..63 = "a" rows, 64..127 = "gate" rows
    img.set_tile(A, lda, B, ldb, M, tm * BM2, [&](int r) { return FWD ? (r < 64 ? tn * 64 + r : N + tn * 64 + (r - 64)) : n0 + r; });
  };

  int v = blockIdx.x;                              // virtual block id: blockIdx.x + it * gridDim.x (same XCD every time)
  if (v >= nwg) return;
  const bool tracing = (dbg & 8) && blockIdx.x == 0 && tid == 0;
  int ti = 0;
  tile_ptrs(xcd_remap(v, nwg));
  img.stage(lds2, 0, 0);
  img.stage(lds2, 64, 1);
  bool first = true;
  while (v < nwg) {
    const int tile = xcd_remap(v, nwg);
    int tm, tn;
    ps_tile_decode(tile, tiles_m, tiles_n, flat_order, tm, tn);
    const int m0 = tm * BM2, n0 = tn * BN;
    f32x16 acc[2][2];
    acc_clear(acc);
    // ---------------- k-loop: three-stage ring, DMA two k-steps ahead (as gemm_nt_256_kernel) ----------------
    // this wave's 64x64 block (MODE 4: columns of h: "a" part for wn = 0, "gate" part for wn = 1)
    const int mw = m0 + wm * 64, nw = FWD ? (wn == 0 ? tn * 64 : N + tn * 64) : n0 + wn * 64;
    const bool edge = m0 + BM2 > M;
    u32x4v pre[NPRE];                              // residual (fp32) / h (bf16 a | gate) pieces of this lane
    u32x4v bvec[2];
    // The epilogue's inputs (NLD loads per wave) are requested three k-steps before the end of the k-loop, right after the
    // last DMA of this tile: they land under the last two k-steps.
    auto preload = [&]() {
      if (BIAS) {
        // MODE 0: this lane's pieces cover columns nw + 8*(lane & 7) .. +7; fp32 modes: nw + 4*(lane & 15) .. +3
        const float* bp = bias + nw + (MODE == 0 ? 8 * (lane & 7) : 4 * (lane & 15));
        PS_GLOAD(bvec[0], bp);
        if (MODE == 0) PS_GLOAD(bvec[1], bp + 4);
      }
      if (MODE == 2) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int u = 0; u < 8; u++) {
            int m = mw + i * 32 + (lane >> 4) + 4 * u; if (m > M - 1) m = M - 1;
            PS_GLOAD(pre[(i * 8 + u) % NPRE], residual + (int64_t)m * ldres + nw + 4 * (lane & 15));
          }
      }
      if (BWD) {
        const u16* h = reinterpret_cast<const u16*>(residual);
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int u = 0; u < 4; u++) {
            int m = mw + i * 32 + (lane >> 3) + 8 * u; if (m > M - 1) m = M - 1;
            const u16* hp = h + (int64_t)m * ldres + nw + 8 * (lane & 7);
            PS_GLOAD(pre[((i * 4 + u) * 2) % NPRE], hp);                  // a
            PS_GLOAD(pre[((i * 4 + u) * 2 + 1) % NPRE], hp + N);          // gate
          }
      }
    };
    int st = 0;
    PS_STAMP();
    for (int kt = 0; kt < nkt; kt++) {
      // stage kt has landed once only the operations issued after its DMA are outstanding (host guarantees nkt >= 5)
      if (kt < 2) { if (first) ps_wait_vm<6>(); else ps_wait_vm<6 + NST>(); }
      else if (kt == nkt - 2) ps_wait_vm<6 + NLD>();          // DMA of the last stage + the epilogue's loads
      else if (kt == nkt - 1) ps_wait_vm<NLD>();
      else ps_wait_vm<6>();
      PS_STAMP();
      __builtin_amdgcn_s_barrier();
      PS_STAMP();
      if (kt + 2 < nkt) { int s2 = st + 2; if (s2 >= 3) s2 -= 3; img.stage(lds2, (kt + 2) * 64, s2); }
      if (NLD > 0 && kt == nkt - 3) preload();
      nt_compute_step<true>(frag, (unsigned)st * (unsigned)(STAGE * 2), acc);
      st = st == 2 ? 0 : st + 1;
      PS_STAMP();
    }
    __builtin_amdgcn_s_barrier();                  // every wave has read its last fragments: all three slots are free
    // The fp32 epilogues hand the accumulators straight to inline-asm ds_write_b128: hipcc does not know the asm reads
    // MFMA results and inserts no wait states (it does for its own v_cvt_pk in the bf16 modes).  The last four MFMAs were
    // issued just before the barrier and take 4 x 32 cycles; without a next tile nothing else sits in between (a
    // one-tile-per-workgroup launch returned stale accumulators once in a few runs).
    if (MODE != 0 && !FWD)
      asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    PS_STAMP();
    // ---------------- epilogue: acc[i][j][4q + e] = C[mw + 32i + l31][nw + 32j + 8q + 4lh + e] ----------------
    // next tile's first two k-steps: in flight during the whole epilogue
    const int vn = v + gridDim.x;
    const bool has_next = vn < nwg;
    if (has_next) {
      tile_ptrs(xcd_remap(vn, nwg));
      img.stage(lds2, 0, 0);
      img.stage(lds2, 64, 1);
    }
    if (NLD > 0) { if (has_next) ps_wait_vm<12>(); else ps_wait_vm<0>(); }          // the epilogue's loads have landed (requested 3 k-steps ago)
    PS_STAMP();
    if (MODE == 0 || FWD) {
      // bf16 payload: 64 rows x 128 B; 16-byte chunk c of row r at chunk c ^ (r & 7)
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            u32x2v pk;
            pk[0] = pack2bf(acc[i][j][4 * q], acc[i][j][4 * q + 1]); pk[1] = pack2bf(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
            const int row = i * 32 + l31, ch = j * 4 + q;
            PS_DSW64(scratch + (unsigned)(row * 128 + ((ch ^ (row & 7)) << 4) + 8 * lh), pk);
          }
      // (SAVED: the wave's own block is not stored: the partner phase below writes the factors into h's place)
      u32x4v o[SAVED ? 1 : 8];
#pragma unroll
      for (int u = 0; u < (SAVED ? 0 : 8); u++) {
        const int row = (lane >> 3) + 8 * u, ch = lane & 7;
        NT_DSREAD(o[u], scratch + (unsigned)(row * 128 + ((ch ^ (row & 7)) << 4)));
      }
      if (!SAVED) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < (SAVED ? 0 : 8); u++) {
        const int m = mw + (lane >> 3) + 8 * u;
        if (BIAS) {          // the accumulators were rounded before the bias: add it and round again (bias GEMMs write fp32 in this model)
          float f[8];
#pragma unroll
          for (int e = 0; e < 4; e++) { f[2 * e] = __uint_as_float(o[u][e] << 16); f[2 * e + 1] = __uint_as_float(o[u][e] & 0xffff0000u); }
#pragma unroll
          for (int e = 0; e < 8; e++) f[e] += __uint_as_float(bvec[e >> 2][e & 3]);
#pragma unroll
          for (int e = 0; e < 4; e++) o[u][e] = pack2bf(f[2 * e], f[2 * e + 1]);
        }
        u16* cp = reinterpret_cast<u16*>(Cv) + (int64_t)m * ldc + nw + 8 * (lane & 7);
        if (m < M) PS_GSTORE(cp, o[u]);
      }
      if (FWD) {
        // g = a * gelu(gate): the partner wave (same rows, other column half) holds the other operand: both blocks are
        // in the scratch areas now; wave wn takes rows 32*wn .. 32*wn + 31 of the pair's 64 rows
        // SAVED: and the two factors of the backward, s = [gelu(gate) | a * gelu'(gate)], into the columns of C that a and gate
        // would have taken: three stores per u, 12 per tile like the eight own-block stores + four g stores of the unsaved form
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const unsigned sa = lds_base + 2u * (unsigned)(STAGE * 2) + (unsigned)(wave & ~1) * 8192u, sg = sa + 8192u;
        u32x4v av[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int row = 32 * wn + (lane >> 3) + 8 * u, ch = lane & 7;
          NT_DSREAD(av[u], sa + (unsigned)(row * 128 + ((ch ^ (row & 7)) << 4)));
          NT_DSREAD(gv[u], sg + (unsigned)(row * 128 + ((ch ^ (row & 7)) << 4)));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        u16* gout = const_cast<u16*>(reinterpret_cast<const u16*>(residual));
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int m = m0 + wm * 64 + 32 * wn + (lane >> 3) + 8 * u;
          u32x4v gg, slo, shi;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float a0 = __uint_as_float(av[u][e] << 16), a1 = __uint_as_float(av[u][e] & 0xffff0000u);
            const float g0 = __uint_as_float(gv[u][e] << 16), g1 = __uint_as_float(gv[u][e] & 0xffff0000u);
            float ge0, ge1, dge0, dge1;
            gelu_pair(g0, ge0, dge0); gelu_pair(g1, ge1, dge1);
            gg[e] = pack2bf(a0 * ge0, a1 * ge1);
            if (SAVED) { slo[e] = pack2bf(ge0, ge1); shi[e] = pack2bf(a0 * dge0, a1 * dge1); }
          }
          u16* gp = gout + (int64_t)m * ldres + tn * 64 + 8 * (lane & 7);
          if (SAVED) {
            u16* sp = reinterpret_cast<u16*>(Cv) + (int64_t)m * ldc + tn * 64 + 8 * (lane & 7);
            if (m < M) { PS_GSTORE(sp, slo); PS_GSTORE(sp + N, shi); }
          }
          if (m < M) PS_GSTORE(gp, gg);
        }
      }
    } else {
      // fp32 payload, one pass per row block i: 32 rows x 256 B; 16-byte chunk c of row r at chunk c ^ (r & 15)
#pragma unroll
      for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            u32x4v w;
#pragma unroll
            for (int e = 0; e < 4; e++) w[e] = __float_as_uint(acc[i][j][4 * q + e]);
            const int ch = j * 8 + 2 * q + lh;
            PS_DSW128(scratch + (unsigned)(l31 * 256 + ((ch ^ (l31 & 15)) << 4)), w);
          }
        if (!BWD) {
          u32x4v o[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int row = (lane >> 4) + 4 * u, ch = lane & 15;
            NT_DSREAD(o[u], scratch + (unsigned)(row * 256 + ((ch ^ (row & 15)) << 4)));
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int m = mw + i * 32 + (lane >> 4) + 4 * u;
            u32x4v ov;
#pragma unroll
            for (int e = 0; e < 4; e++) {
              float t = __uint_as_float(o[u][e]);
              if (BIAS) t += __uint_as_float(bvec[0][e]);
              if (MODE == 2) t += __uint_as_float(pre[(i * 8 + u) % NPRE][e]);
              ov[e] = __float_as_uint(t);
            }
            float* cp = reinterpret_cast<float*>(Cv) + (int64_t)m * ldc + nw + 4 * (lane & 15);
            if (m < M) PS_GSTORE(cp, ov);
          }
        } else {
          // GEGLU backward: pieces of 8 columns (two adjacent 16-byte chunks of dg), h = [a | gate]
          u32x4v o[4][2];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int row = (lane >> 3) + 8 * u, ch = 2 * (lane & 7);
            NT_DSREAD(o[u][0], scratch + (unsigned)(row * 256 + ((ch ^ (row & 15)) << 4)));
            NT_DSREAD(o[u][1], scratch + (unsigned)(row * 256 + (((ch + 1) ^ (row & 15)) << 4)));
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int m = mw + i * 32 + (lane >> 3) + 8 * u;
            const u32x4v av = pre[((i * 4 + u) * 2) % NPRE], gv = pre[((i * 4 + u) * 2 + 1) % NPRE];
            u32x4v da, dgt;
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const float d0 = __uint_as_float(o[u][e >> 1][2 * (e & 1)]), d1 = __uint_as_float(o[u][e >> 1][2 * (e & 1) + 1]);
              const float a0 = __uint_as_float(av[e] << 16), a1 = __uint_as_float(av[e] & 0xffff0000u);
              const float g0 = __uint_as_float(gv[e] << 16), g1 = __uint_as_float(gv[e] & 0xffff0000u);
              if (SAVED) {          // av = s_lo = gelu(gate), gv = s_hi = a * gelu'(gate): the forward's saved factors
                da[e] = pack2bf(d0 * a0, d1 * a1);
                dgt[e] = pack2bf(d0 * g0, d1 * g1);
                continue;
              }
              float ge0, dge0, ge1, dge1;
              gelu_pair(g0, ge0, dge0); gelu_pair(g1, ge1, dge1);
              da[e] = pack2bf(d0 * ge0, d1 * ge1);
              dgt[e] = pack2bf(d0 * a0 * dge0, d1 * a1 * dge1);
            }
            u16* cp = reinterpret_cast<u16*>(Cv) + (int64_t)m * ldc + nw + 8 * (lane & 7);
            if (m < M) { PS_GSTORE(cp, da); PS_GSTORE(cp + N, dgt); }
          }
        }
      }
    }
    if (edge) ps_wait_vm<0>();
    PS_STAMP();
    first = false;
    v = vn;
  }
}


// ---------------------------------------------------------------------------------------------------------
// PERSISTENT NT kernel with 256 x 256 tiles (bf16 output, N % 256 == 0): the k-loop of these GEMMs is bound by the
// L2 -> LDS path per CU, and a 256x256 tile moves 2/3 of the operand bytes per flop of a 256x128 one.  8 wavefronts as
// 4 (m) x 2 (n), each 64 x 128 = 2 x 4 accumulators (128 VGPRs, operands swapped: lane = row); k-steps of 32 in FIVE
// slots of 32 KiB (DMA three to four steps ahead, software-pipelined fragment reads: see the k-loop); the next tile's first
// three stages are issued before the epilogue, which uses slots 3 and 4 as 8 KiB of scratch per wave (two passes of 32 rows x
// 256 B).  vmcnt per wave: 4 loads per stage, 16 stores per tile.
// ---------------------------------------------------------------------------------------------------------
// GEGLU = true: fused FF1 + GEGLU forward (see mca_gemm_nt_geglu_fwd): B = W1 [2*N, K] with N = ip, a column tile = 128 "a"
// rows + the 128 "gate" rows of the same columns (wave column wn = 0 holds a, wn = 1 gate), C = h [M, 2*N], G = g [M, N].
// SAVED (with GEGLU): C = s = [gelu(gate) | a * gelu'(gate)], the backward's factors, in h's place (mca_gemm_nt_geglu_fwd_saved):
// the 16 own-block stores of a tile are not made and the partner phase stores s_lo, s_hi and g: 24 stores as before.
// CB (plain form only, mca_gemm_nt_cb): C is stored column-blocked, [N / 64][M][64] with `ldc` = cbs elements between the 64-column
// slabs: column n of row m at C + (n / 64) * cbs + m * 64 + n % 64.  Only the address of the 16 stores moves: a lane's 16 bytes stay
// inside one slab row and eight lanes fill its 128 bytes; NST and every wait count are those of the row-major store.
template <bool GEGLU, bool SAVED = false, bool CB = false>
__global__ __launch_bounds__(512) void gemm_nt_persist256_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, u16* __restrict__ C, int64_t ldc,
    u16* __restrict__ G, int64_t ldg, int M, int N, int K, int tiles_n, int nwg, int dbg) {
  extern __shared__ __attribute__((aligned(16))) u16 lds2[];
  constexpr int NST = GEGLU ? 24 : 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  const int nkt = K / 32;
  const int tiles_m = nwg / tiles_n;
  const unsigned lds_base = lds_addr(lds2);
  const unsigned scratch = lds_base + 3u * (unsigned)(P2_STAGE * 2) + (unsigned)wave * 8192u;          // slot 3 and the 32 KiB after it

  // fragment byte addresses inside a stage: row R (64-byte rows), k16-step ks: R*64 + ((lh ^ sw(R)) << 4) ^ (32*ks)
  unsigned fa_addr[2], fb_addr[4];
#pragma unroll
  for (int i = 0; i < 2; i++) { const int r = wm * 64 + i * 32 + l31; fa_addr[i] = lds_base + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }
#pragma unroll
  for (int j = 0; j < 4; j++) { const int r = wn * 128 + j * 32 + l31; fb_addr[j] = lds_base + 256u * 64u + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }

  const u16* ga[2];
  const u16* gb[2];
  auto tile_ptrs = [&](int tile) {
    int tm, tn;
    ps_tile_decode(tile, tiles_m, tiles_n, 0, tm, tn);
    const int m0 = tm * 256, n0 = tn * 256;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int p = (i * 8 + wave) * 64 + lane, r = p >> 2, c = (p & 3) ^ gl_sw<32>(r);
      int ra = m0 + r; if (ra > M - 1) ra = M - 1;
      ga[i] = A + (int64_t)ra * lda + c * 8;
      // N % 256 == 0 (GEGLU: N % 128 == 0): no clamp.  GEGLU: tile rows 0..127 = "a" rows, 128..255 = "gate" rows
      const int rb = GEGLU ? (r < 128 ? tn * 128 + r : N + tn * 128 + (r - 128)) : n0 + r;
      gb[i] = B + (int64_t)rb * ldb + c * 8;
    }
  };
  auto stage = [&](int k0, int st) {
    u16* base = lds2 + st * P2_STAGE;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      lds_dma16(ga[i] + k0, base + (i * 8 + wave) * 512);
      lds_dma16(gb[i] + k0, base + 256 * 32 + (i * 8 + wave) * 512);
    }
  };

  int v = blockIdx.x;
  if (v >= nwg) return;
  tile_ptrs(xcd_remap(v, nwg));
  stage(0, 0); stage(32, 1); stage(64, 2);
  bool first = true;
  while (v < nwg) {
    const int tile = xcd_remap(v, nwg);
    int tm, tn;
    ps_tile_decode(tile, tiles_m, tiles_n, 0, tm, tn);
    const int m0 = tm * 256, n0 = tn * 256;
    f32x16 acc[2][4];
    acc_clear(acc);
    // FIVE slots of 32 KiB (the fifth is the half of the epilogue scratch that a k-loop does not need): stage kt lives in slot
    // kt % 5, stages 0..2 were issued by the previous tile's epilogue (or the prologue), stage 3 goes out at the top of the tile and
    // stage kt + 4 in the middle of step kt.  The step is the software-pipelined one of gemm_tile.h (T256_GROUP_READING), shared
    // with tn_256x256_tile; the read, the MFMA and the wait ladder are this kernel's.
    // vmcnt, in issue order per wave: S0 S1 S2 [NST epilogue stores of the previous tile] S3 S4 ...: a stage has landed once only
    // the operations issued after its DMA are outstanding (host: nkt >= 6).
    u32x4v fa[2][2], fb[2][4];          // [k16-step][block]
#define P2_RA(KS, I, SO) NT_DSREAD(fa[KS][I], (fa_addr[I] + (SO)) ^ (32u * (KS))); T256_SB
#define P2_RB(KS, J, SO) NT_DSREAD(fb[KS][J], (fb_addr[J] + (SO)) ^ (32u * (KS))); T256_SB
#define P2_MM(KS, I, J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&fb[KS][J]), \
                                                                            *reinterpret_cast<const bf16x8*>(&fa[KS][I]), acc[I][J], 0, 0, 0); T256_SB
#define P2_GROUP_READING(KS, KN, SO, MID) T256_GROUP_READING(P2_RA, P2_RB, P2_MM, KS, KN, SO, MID)
    if (first) ps_wait_vm<8>(); else ps_wait_vm<8 + NST>();          // S0 has landed
    __builtin_amdgcn_s_barrier();                                     // ... for everyone, and every wave has left the previous epilogue
    stage(96, 3);
    T256_SB
    T256_FIRST_READS(P2_RA, P2_RB)
    int slot = 0, prev = 4;
    for (int kt = 0; kt + 1 < nkt; kt++) {
      const unsigned so = (unsigned)slot * (unsigned)(P2_STAGE * 2);
      const int nxt = slot == 4 ? 0 : slot + 1;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
      P2_GROUP_READING(0, 1, so, )
      // stage kt + 1 has landed once only what was issued after it is outstanding; past the barrier every wave has finished with
      // stage kt - 1, whose slot takes stage kt + 4
      if (kt < 2) { if (first) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory"); else { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); ps_wait_vm<8 + NST>(); } }
      else if (kt + 3 < nkt) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
      else if (kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      T256_SB
      const unsigned son = (unsigned)nxt * (unsigned)(P2_STAGE * 2);
      const bool fetch = kt + 4 < nkt;
      P2_GROUP_READING(1, 0, son, if (fetch) stage((kt + 4) * 32, prev); T256_SB)
      prev = slot; slot = nxt;
    }
    {          // the last stage: nothing left to wait for or to fetch
      const unsigned so = (unsigned)slot * (unsigned)(P2_STAGE * 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
      P2_GROUP_READING(0, 1, so, )
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
      T256_GROUP(P2_MM, 1)
    }
#undef P2_RA
#undef P2_RB
#undef P2_MM
#undef P2_GROUP_READING
    __builtin_amdgcn_s_barrier();                  // every wave has read its last fragments: all five slots are free
    // ---------------- epilogue: acc[i][j][4q + e] = C[mw + 32i + l31][nw + 32j + 8q + 4lh + e] ----------------
    const int mw = m0 + wm * 64, nw = GEGLU ? (wn == 0 ? tn * 128 : N + tn * 128) : n0 + wn * 128;
    const bool edge = m0 + 256 > M;
    const int vn = v + gridDim.x;
    const bool has_next = vn < nwg;
    if (has_next) {
      tile_ptrs(xcd_remap(vn, nwg));
      stage(0, 0); stage(32, 1); stage(64, 2);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
      // bf16 payload of row block i: 32 rows x 256 B; 16-byte chunk c of row r at chunk c ^ (r & 15)
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          u32x2v pk;
          pk[0] = pack2bf(acc[i][j][4 * q], acc[i][j][4 * q + 1]); pk[1] = pack2bf(acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
          const int ch = j * 4 + q;
          PS_DSW64(scratch + (unsigned)(l31 * 256 + ((ch ^ (l31 & 15)) << 4) + 8 * lh), pk);
        }
      u32x4v o[SAVED ? 1 : 8];
#pragma unroll
      for (int u = 0; u < (SAVED ? 0 : 8); u++) {
        const int row = (lane >> 4) + 4 * u, ch = lane & 15;
        NT_DSREAD(o[u], scratch + (unsigned)(row * 256 + ((ch ^ (row & 15)) << 4)));
      }
      if (!SAVED) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < (SAVED ? 0 : 8); u++) {
        const int m = mw + i * 32 + (lane >> 4) + 4 * u;
        u16* cp;
        if constexpr (CB) cp = C + (int64_t)((nw >> 6) + ((lane & 15) >> 3)) * ldc + (int64_t)m * 64 + 8 * (lane & 7);
        else cp = C + (int64_t)m * ldc + nw + 8 * (lane & 15);
        if (m < M) PS_GSTORE(cp, o[u]);
      }
      if (GEGLU) {
        // g = a * gelu(gate): the partner wave (same rows, other column half) holds the other operand; both row blocks are
        // in the scratch areas now.  Wave wn takes rows 16*wn .. 16*wn + 15 of the pair's 32 rows.
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const unsigned sa = lds_base + 3u * (unsigned)(P2_STAGE * 2) + (unsigned)(wave & ~1) * 8192u, sg = sa + 8192u;
        u32x4v av[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int row = 16 * wn + (lane >> 4) + 4 * u, ch = lane & 15;
          NT_DSREAD(av[u], sa + (unsigned)(row * 256 + ((ch ^ (row & 15)) << 4)));
          NT_DSREAD(gv[u], sg + (unsigned)(row * 256 + ((ch ^ (row & 15)) << 4)));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int m = m0 + wm * 64 + i * 32 + 16 * wn + (lane >> 4) + 4 * u;
          u32x4v gg, slo, shi;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float a0 = __uint_as_float(av[u][e] << 16), a1 = __uint_as_float(av[u][e] & 0xffff0000u);
            const float g0 = __uint_as_float(gv[u][e] << 16), g1 = __uint_as_float(gv[u][e] & 0xffff0000u);
            float ge0, ge1, dge0, dge1;
            gelu_pair(g0, ge0, dge0); gelu_pair(g1, ge1, dge1);
            gg[e] = pack2bf(a0 * ge0, a1 * ge1);
            if (SAVED) { slo[e] = pack2bf(ge0, ge1); shi[e] = pack2bf(a0 * dge0, a1 * dge1); }
          }
          u16* gp = G + (int64_t)m * ldg + tn * 128 + 8 * (lane & 15);
          if (SAVED) {
            u16* sp = C + (int64_t)m * ldc + tn * 128 + 8 * (lane & 15);
            if (m < M) { PS_GSTORE(sp, slo); PS_GSTORE(sp + N, shi); }
          }
          if (m < M) PS_GSTORE(gp, gg);
        }
        if (i == 0) asm volatile("s_barrier" ::: "memory");          // the partner has read this row block: scratch may be overwritten
      }
    }
    if (edge) ps_wait_vm<0>();
    first = false;
    v = vn;
  }
}

// ---------------------------------------------------------------------------------------------------------
// FULL-ROW NT kernel (N = 512 exactly): one workgroup computes 128 WHOLE rows of C = A.B^T, so the LayerNorm that consumes C
// runs on the tile before it leaves the CU and C itself is never written.  8 wavefronts as 2 (m) x 4 (n), each 64 x 128 = 2 x 4
// accumulators (the per-wavefront shape of gemm_nt_persist256_kernel, operands NOT swapped: lane = column, register = row, k16-steps
// ascending, i.e. the fp32 chain of gemm_nt_glds_kernel / gemm_nt_256_kernel).  k-steps of 32 through a ring of three 40 KiB stages
// (A image [128][32], B image [512][32], the gl_sw<32> swizzle; 1 + 4 loads per wave and stage), DMA two to three steps ahead, one
// barrier per step behind a counted vmcnt; the step is the software-pipelined one of gemm_tile.h (T256_GROUP_READING).
// vmcnt per wave, in issue order: S0 S1 S2 | S3 (middle of step 0) | S4 ...: stage kt + 1 has landed once at most the 5 loads of
// stage kt + 2 are outstanding (host: K >= 96, three steps).  The last step leaves nothing in flight: the epilogue is plain C++.
// Epilogue, four passes of 32 rows through 64.5 KiB of the ring: pass p takes rows 16 (p & 1) .. + 15 of row block p >> 1 of both
// wave rows (registers 8 (p & 1) .. + 7 of acc[p >> 1][.]), so every wave writes in every pass; then wave w owns rows 4 w .. 4 w + 3
// of the pass, two at a time in the lane layout of the trunk LayerNorm kernels (element (lane + 64 i) * 4, NI = 2).
// The epilogue (mca_gemm_nt_res_lnbwd): dy = A.B^T (+ residual) stays on chip; the row body of ln_bwd_trunk_kernel (ln_rows.h) makes dx
// (fp32), its bf16 copy and the lane's dgamma partials; block reduction, then one atomic per column and workgroup.  dx may be the
// residual: a row is read and written by one wavefront, the reads first.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void gemm_nt_rows_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, const float* residual, int64_t ldres,
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const float* __restrict__ gamma, float* dx, int64_t lddx, u16* __restrict__ dx_bf16, int64_t ld_bf16, float* __restrict__ dgamma,
    int M, int K, int nwg) {
  extern __shared__ __attribute__((aligned(16))) u16 lds2[];
  constexpr unsigned STAGE_BYTES = ROWS_STAGE * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, lh = lane >> 5;
  const int nkt = K / ROWS_BK;
  const int m0 = xcd_remap(blockIdx.x, nwg) * ROWS_BM;
  const unsigned lds_base = lds_addr(lds2);

  // fragment byte addresses inside a stage, as in gemm_nt_persist256_kernel: row R (64-byte rows), k16-step ks
  unsigned fa_addr[2], fb_addr[4];
#pragma unroll
  for (int i = 0; i < 2; i++) { const int r = wm * 64 + i * 32 + l31; fa_addr[i] = lds_base + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }
#pragma unroll
  for (int j = 0; j < 4; j++) { const int r = wn * 128 + j * 32 + l31; fb_addr[j] = lds_base + (unsigned)(ROWS_BM * 64) + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }

  const u16* ga;
  const u16* gb[4];
  {
    const int p = wave * 64 + lane, r = p >> 2, c = (p & 3) ^ gl_sw<32>(r);
    int ra = m0 + r; if (ra > M - 1) ra = M - 1;          // rows past M: clamped (loaded and computed, never stored)
    ga = A + (int64_t)ra * lda + c * 8;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p = (i * 8 + wave) * 64 + lane, r = p >> 2, c = (p & 3) ^ gl_sw<32>(r);          // r < 512 = N: no clamp
    gb[i] = B + (int64_t)r * ldb + c * 8;
  }
  auto stage = [&](int k0, int st) {
    u16* base = lds2 + st * ROWS_STAGE;
    lds_dma16(ga + k0, base + wave * 512);
#pragma unroll
    for (int i = 0; i < 4; i++) lds_dma16(gb[i] + k0, base + ROWS_BM * ROWS_BK + (i * 8 + wave) * 512);
  };

  f32x16 acc[2][4];
  acc_clear(acc);
  stage(0, 0); stage(ROWS_BK, 1); stage(2 * ROWS_BK, 2);
  u32x4v fa[2][2], fb[2][4];          // [k16-step][block]
#define RW_RA(KS, I, SO) NT_DSREAD(fa[KS][I], (fa_addr[I] + (SO)) ^ (32u * (KS))); T256_SB
#define RW_RB(KS, J, SO) NT_DSREAD(fb[KS][J], (fb_addr[J] + (SO)) ^ (32u * (KS))); T256_SB
#define RW_MM(KS, I, J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&fa[KS][I]), \
                                                                            *reinterpret_cast<const bf16x8*>(&fb[KS][J]), acc[I][J], 0, 0, 0); T256_SB
#define RW_GROUP_READING(KS, KN, SO, MID) T256_GROUP_READING(RW_RA, RW_RB, RW_MM, KS, KN, SO, MID)
  ps_wait_vm<10>();                                  // S0 has landed
  __builtin_amdgcn_s_barrier();                      // ... for everyone
  T256_SB
  T256_FIRST_READS(RW_RA, RW_RB)
  int slot = 0;
  for (int kt = 0; kt + 1 < nkt; kt++) {
    const unsigned so = (unsigned)slot * STAGE_BYTES;
    const int nxt = slot == 2 ? 0 : slot + 1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    RW_GROUP_READING(0, 1, so, )
    // stage kt + 1 has landed once only stage kt + 2 is outstanding; past the barrier every wave has read all of stage kt, whose
    // slot takes stage kt + 3
    if (kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    T256_SB
    const unsigned son = (unsigned)nxt * STAGE_BYTES;
    const bool fetch = kt + 3 < nkt;
    RW_GROUP_READING(1, 0, son, if (fetch) stage((kt + 3) * ROWS_BK, slot); T256_SB)
    slot = nxt;
  }
  {          // the last stage: nothing left to wait for or to fetch
    const unsigned so = (unsigned)slot * STAGE_BYTES;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    RW_GROUP_READING(0, 1, so, )
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    T256_GROUP(RW_MM, 1)
  }
#undef RW_RA
#undef RW_RB
#undef RW_MM
#undef RW_GROUP_READING
  __syncthreads();                                   // every wave has read its last fragments: the ring is free

  // ---------------- epilogue: acc[i][j][r] = C[m0 + wm * 64 + i * 32 + acc_row(r, lh)][wn * 128 + j * 32 + l31] ----------------
  float* cs = reinterpret_cast<float*>(lds2);        // [32][ROWS_CS_LD]
  float4 gm[2], dg[2];
#pragma unroll
  for (int i = 0; i < 2; i++) { gm[i] = *reinterpret_cast<const float4*>(gamma + (lane + 64 * i) * 4); dg[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
  const float inv_cols = 1.f / (float)ROWS_N;
  // x, the residual, dx and its copy are streamed once: non-temporal, so that they do not evict B (up to 2.9 MiB, re-read by every
  // workgroup) from the L2
  auto ld4 = [](const float* p) { const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); return make_float4(t[0], t[1], t[2], t[3]); };
  auto st4 = [](float* p, const float4& o) { __builtin_nontemporal_store(f32x4{o.x, o.y, o.z, o.w}, reinterpret_cast<f32x4*>(p)); };
  auto st4b = [](u16* p, const float4& o) { const uint2 pk = ln_pack4bf(o); __builtin_nontemporal_store(u32x2v{pk.x, pk.y}, reinterpret_cast<u32x2v*>(p)); };
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const int bi = p >> 1, half = p & 1;
    // this wave's four rows of the pass, two pairs q of consecutive rows of C.  Their x and residual are requested before the tile
    // goes through LDS (rows past M clamped: loaded, never used), so they travel under the LDS pass and its two barriers.
    // Not a race in the in-place case (dx == residual): a clamped load reads row M - 1, which the wave owning that row may be
    // storing at the same moment, but the loop below skips every row past M, so what such a load returned is never looked at.
    // A row below M is loaded here and stored below by the same wave, the loads first.
    float4 xq[2][2][2], rq[2][2][2];          // [q][row a / b][i]
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int lr = wave * 4 + q * 2;
      const int mrow = m0 + (lr >> 4) * 64 + bi * 32 + half * 16 + (lr & 15);
      const int64_t r0 = mrow < M ? mrow : M - 1, r1 = mrow + 1 < M ? mrow + 1 : r0;
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        xq[q][0][i] = ld4(x + r0 * ldx + c); xq[q][1][i] = ld4(x + r1 * ldx + c);
        if (residual) { rq[q][0][i] = ld4(residual + r0 * ldres + c); rq[q][1][i] = ld4(residual + r1 * ldres + c); }
        else { rq[q][0][i] = make_float4(0.f, 0.f, 0.f, 0.f); rq[q][1][i] = make_float4(0.f, 0.f, 0.f, 0.f); }
      }
    }
    if (p) __syncthreads();                          // the previous pass has been read
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int rr = 0; rr < 8; rr++) cs[(wm * 16 + acc_row(rr, lh)) * ROWS_CS_LD + wn * 128 + j * 32 + l31] = acc[bi][j][half * 8 + rr];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int lr = wave * 4 + q * 2;                // rows lr, lr + 1 of the pass
      const int mrow = m0 + (lr >> 4) * 64 + bi * 32 + half * 16 + (lr & 15);
      if (mrow >= M) continue;
      const bool two = mrow + 1 < M;
      const int64_t r0 = mrow, r1 = two ? r0 + 1 : r0;
      const float* ca = cs + lr * ROWS_CS_LD;
      const float* cb = cs + (two ? lr + 1 : lr) * ROWS_CS_LD;
      float4 xa[2], xb[2], da[2], db[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        xa[i] = xq[q][0][i]; da[i] = *reinterpret_cast<const float4*>(ca + c);
        xb[i] = xq[q][1][i]; db[i] = *reinterpret_cast<const float4*>(cb + c);
      }
      if (residual) {                                 // dy = A.B^T + residual, the add of the plain GEMM's epilogue
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const float4 ta = rq[q][0][i], tb = rq[q][1][i];
          da[i].x += ta.x; da[i].y += ta.y; da[i].z += ta.z; da[i].w += ta.w;
          db[i].x += tb.x; db[i].y += tb.y; db[i].z += tb.z; db[i].w += tb.w;
        }
      }
      const float ma = mean_in[r0], ra = rstd_in[r0], mb = mean_in[r1], rb = rstd_in[r1];
      float s1a, s2a, s1b, s2b;
      ln_bwd_rows_stats<2>(xa, xb, da, db, gm, dg, ma, ra, mb, rb, two, inv_cols, s1a, s2a, s1b, s2b);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        float4 o = ln_bwd_row_dx(da[i], xa[i], ra, s1a, s2a);
        st4(dx + r0 * lddx + c, o);
        st4b(dx_bf16 + r0 * ld_bf16 + c, o);
        if (two) {
          o = ln_bwd_row_dx(db[i], xb[i], rb, s1b, s2b);
          st4(dx + r1 * lddx + c, o);
          st4b(dx_bf16 + r1 * ld_bf16 + c, o);
        }
      }
    }
  }
  // block reduction of the dgamma partials through LDS, then one atomic per column and workgroup
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; i++) *reinterpret_cast<float4*>(cs + wave * ROWS_N + (lane + 64 * i) * 4) = dg[i];
  __syncthreads();
  float t = cs[tid];
#pragma unroll
  for (int w = 1; w < 8; w++) t += cs[w * ROWS_N + tid];
  if (t != 0.f) atomicAdd(dgamma + tid, t);
}

// ---------------------------------------------------------------------------------------------------------
// The TALL form of the full-row kernel: 160 whole rows per workgroup (mca_gemm_nt_res_lnbwd_tall, where the height rule of
// gemm_plan.h picks it: 81,216 rows are 508 tiles = two rounds on 256 CUs instead of 635 = three).  Same contract, same fp32 chains
// (operands not swapped, k16-steps ascending), same row body; only the tile differs.  8 wavefronts as 1 (m) x 8 (n): wave w owns all
// 160 rows x columns 64 w .. 64 w + 63 = 5 x 2 accumulators, so per k16-step it reads 5 A + 2 B fragments for 10 MFMAs.
// Ring: three stages of (A image [160][32], B image [512][32]), 42 KiB each.  The B image is 4 loads per wave and stage as above;
// the A image is 640 16-byte pieces = ten wave-loads, one per wave and a second one for waves 0 and 1 (pieces 512 .. 639, rows
// 128 .. 159).  So waves 0 / 1 have SIX loads per stage in flight and waves 2 .. 7 FIVE, and every counted wait has two immediates
// behind a wave-uniform branch (`six`).  vmcnt per wave, in issue order: S0 S1 S2 | S3 (middle of step 0) | S4 ...
//   after the prologue 3 stages are outstanding (18 / 15 loads); S0 has landed once at most S1 + S2 are:  vmcnt(12) / vmcnt(10)
//   in step kt, S(kt + 2) is the newest stage issued; S(kt + 1) has landed once at most S(kt + 2) is out:  vmcnt(6)  / vmcnt(5)
//   in the last step but one nothing newer than S(kt + 1) exists:                                           vmcnt(0)
// (vmcnt(5) would do for waves 0 / 1 too, one load late; vmcnt(6) on waves 2 .. 7 would let them pass with the newest load of
// S(kt + 1) still in flight.)  Each wave waits for its own loads only; the barrier behind the wait completes the stage for everyone.
// Epilogue: five passes, pass p = row block p: every wave writes its 64 columns x 32 rows (acc[p][0..1], all 16 registers) into cs
// at row acc_row(r, lh); then wave w owns rows 4 w .. 4 w + 3 of the pass, two at a time, exactly as above.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void gemm_nt_rows160_kernel(
    const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb, const float* residual, int64_t ldres,
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const float* __restrict__ gamma, float* dx, int64_t lddx, u16* __restrict__ dx_bf16, int64_t ld_bf16, float* __restrict__ dgamma,
    int M, int K, int nwg) {
  extern __shared__ __attribute__((aligned(16))) u16 lds2[];
  constexpr unsigned STAGE_BYTES = ROWS160_STAGE * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const bool six = __builtin_amdgcn_readfirstlane(wave) < 2;          // this wave carries a second A load (wave-uniform)
  const int nkt = K / ROWS_BK;
  const int m0 = xcd_remap(blockIdx.x, nwg) * ROWS160_BM;
  const unsigned lds_base = lds_addr(lds2);

  // fragment byte addresses inside a stage: row R (64-byte rows), k16-step ks: R * 64 + ((lh ^ sw(R)) << 4) ^ (32 * ks)
  unsigned fa_addr[5], fb_addr[2];
#pragma unroll
  for (int i = 0; i < 5; i++) { const int r = i * 32 + l31; fa_addr[i] = lds_base + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }
#pragma unroll
  for (int j = 0; j < 2; j++) { const int r = wave * 64 + j * 32 + l31; fb_addr[j] = lds_base + (unsigned)(ROWS160_BM * 64) + (unsigned)(r * 64 + ((lh ^ gl_sw<32>(r)) << 4)); }

  const u16* ga[2];          // pieces wave * 64 + lane (rows 0 .. 127) and, waves 0 / 1 only, 512 + wave * 64 + lane (rows 128 .. 159)
  const u16* gb[4];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int p = (i * 8 + (i ? wave & 1 : wave)) * 64 + lane, r = p >> 2, c = (p & 3) ^ gl_sw<32>(r);
    int ra = m0 + r; if (ra > M - 1) ra = M - 1;          // rows past M: clamped (loaded and computed, never stored)
    ga[i] = A + (int64_t)ra * lda + c * 8;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int p = (i * 8 + wave) * 64 + lane, r = p >> 2, c = (p & 3) ^ gl_sw<32>(r);          // r < 512 = N: no clamp
    gb[i] = B + (int64_t)r * ldb + c * 8;
  }
  auto stage = [&](int k0, int st) {
    u16* base = lds2 + st * ROWS160_STAGE;
    lds_dma16(ga[0] + k0, base + wave * 512);
    if (six) lds_dma16(ga[1] + k0, base + (8 + wave) * 512);
#pragma unroll
    for (int i = 0; i < 4; i++) lds_dma16(gb[i] + k0, base + ROWS160_BM * ROWS_BK + (i * 8 + wave) * 512);
  };

  f32x16 acc[5][2];
#pragma unroll
  for (int i = 0; i < 5; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  stage(0, 0); stage(ROWS_BK, 1); stage(2 * ROWS_BK, 2);
  u32x4v fa[2][5], fb[2][2];          // [k16-step][block]
#define R160_RA(KS, I, SO) NT_DSREAD(fa[KS][I], (fa_addr[I] + (SO)) ^ (32u * (KS))); T256_SB
#define R160_RB(KS, J, SO) NT_DSREAD(fb[KS][J], (fb_addr[J] + (SO)) ^ (32u * (KS))); T256_SB
#define R160_MM(KS, I, J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&fa[KS][I]), \
                                                                              *reinterpret_cast<const bf16x8*>(&fb[KS][J]), acc[I][J], 0, 0, 0); T256_SB
// the software-pipelined k-step of gemm_tile.h (T256_GROUP_READING) for 5 x 2 blocks: the 10 MFMAs of k16-step KS with the 7 fragment
// reads of k16-step KN in their gaps, one per gap; MID - the DMA of the stage three steps ahead - behind the first MFMA.  A block
// is read again as late after its last MFMA of the group before as the order allows (the B blocks and A block 4 close a group).
#define R160_FIRST_READS R160_RA(0, 0, 0u) R160_RB(0, 0, 0u) R160_RB(0, 1, 0u) R160_RA(0, 1, 0u) R160_RA(0, 2, 0u) R160_RA(0, 3, 0u) R160_RA(0, 4, 0u)
#define R160_GROUP_READING(KS, KN, SO, MID)                                                                                       \
  R160_MM(KS, 0, 0) MID R160_RA(KN, 0, SO) R160_MM(KS, 0, 1) R160_RA(KN, 1, SO) R160_MM(KS, 1, 0) R160_RA(KN, 2, SO)                \
  R160_MM(KS, 1, 1) R160_RA(KN, 3, SO) R160_MM(KS, 2, 0) R160_RB(KN, 0, SO) R160_MM(KS, 2, 1) R160_RB(KN, 1, SO)                    \
  R160_MM(KS, 3, 0) R160_RA(KN, 4, SO) R160_MM(KS, 3, 1) R160_MM(KS, 4, 0) R160_MM(KS, 4, 1)
#define R160_GROUP(KS) R160_MM(KS, 0, 0) R160_MM(KS, 0, 1) R160_MM(KS, 1, 0) R160_MM(KS, 1, 1) R160_MM(KS, 2, 0) R160_MM(KS, 2, 1) \
  R160_MM(KS, 3, 0) R160_MM(KS, 3, 1) R160_MM(KS, 4, 0) R160_MM(KS, 4, 1)
  if (six) ps_wait_vm<12>(); else ps_wait_vm<10>();          // S0 has landed: at most S1 + S2 (6 / 5 loads each) are outstanding
  __builtin_amdgcn_s_barrier();                              // ... for everyone
  T256_SB
  R160_FIRST_READS
  int slot = 0;
  for (int kt = 0; kt + 1 < nkt; kt++) {
    const unsigned so = (unsigned)slot * STAGE_BYTES;
    const int nxt = slot == 2 ? 0 : slot + 1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    R160_GROUP_READING(0, 1, so, )
    // stage kt + 1 has landed once only stage kt + 2 (6 loads of waves 0 / 1, 5 of the others) is outstanding; past the barrier
    // every wave has read all of stage kt, whose slot takes stage kt + 3
    if (kt + 2 < nkt) {
      if (six) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
    } else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    T256_SB
    const unsigned son = (unsigned)nxt * STAGE_BYTES;
    const bool fetch = kt + 3 < nkt;
    R160_GROUP_READING(1, 0, son, if (fetch) stage((kt + 3) * ROWS_BK, slot); T256_SB)
    slot = nxt;
  }
  {          // the last stage: nothing left to wait for or to fetch
    const unsigned so = (unsigned)slot * STAGE_BYTES;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    R160_GROUP_READING(0, 1, so, )
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    R160_GROUP(1)
  }
#undef R160_RA
#undef R160_RB
#undef R160_MM
#undef R160_FIRST_READS
#undef R160_GROUP_READING
#undef R160_GROUP
  __syncthreads();                                   // every wave has read its last fragments: the ring is free

  // ---------------- epilogue: acc[i][j][r] = C[m0 + i * 32 + acc_row(r, lh)][wave * 64 + j * 32 + l31] ----------------
  float* cs = reinterpret_cast<float*>(lds2);        // [32][ROWS_CS_LD]
  float4 gm[2], dg[2];
#pragma unroll
  for (int i = 0; i < 2; i++) { gm[i] = *reinterpret_cast<const float4*>(gamma + (lane + 64 * i) * 4); dg[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
  const float inv_cols = 1.f / (float)ROWS_N;
  // x, the residual, dx and its copy are streamed once: non-temporal, as in gemm_nt_rows_kernel
  auto ld4 = [](const float* p) { const f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); return make_float4(t[0], t[1], t[2], t[3]); };
  auto st4 = [](float* p, const float4& o) { __builtin_nontemporal_store(f32x4{o.x, o.y, o.z, o.w}, reinterpret_cast<f32x4*>(p)); };
  auto st4b = [](u16* p, const float4& o) { const uint2 pk = ln_pack4bf(o); __builtin_nontemporal_store(u32x2v{pk.x, pk.y}, reinterpret_cast<u32x2v*>(p)); };
#pragma unroll
  for (int p = 0; p < 5; p++) {
    // this wave's four rows of the pass, two pairs q of consecutive rows of C, their x and residual requested before the tile goes
    // through LDS (rows past M clamped: loaded, never used; the in-place case: see gemm_nt_rows_kernel)
    float4 xq[2][2][2], rq[2][2][2];          // [q][row a / b][i]
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int mrow = m0 + p * 32 + wave * 4 + q * 2;
      const int64_t r0 = mrow < M ? mrow : M - 1, r1 = mrow + 1 < M ? mrow + 1 : r0;
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        xq[q][0][i] = ld4(x + r0 * ldx + c); xq[q][1][i] = ld4(x + r1 * ldx + c);
        if (residual) { rq[q][0][i] = ld4(residual + r0 * ldres + c); rq[q][1][i] = ld4(residual + r1 * ldres + c); }
        else { rq[q][0][i] = make_float4(0.f, 0.f, 0.f, 0.f); rq[q][1][i] = make_float4(0.f, 0.f, 0.f, 0.f); }
      }
    }
    if (p) __syncthreads();                          // the previous pass has been read
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rr = 0; rr < 16; rr++) cs[acc_row(rr, lh) * ROWS_CS_LD + wave * 64 + j * 32 + l31] = acc[p][j][rr];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int lr = wave * 4 + q * 2;                // rows lr, lr + 1 of the pass
      const int mrow = m0 + p * 32 + lr;
      if (mrow >= M) continue;
      const bool two = mrow + 1 < M;
      const int64_t r0 = mrow, r1 = two ? r0 + 1 : r0;
      const float* ca = cs + lr * ROWS_CS_LD;
      const float* cb = cs + (two ? lr + 1 : lr) * ROWS_CS_LD;
      float4 xa[2], xb[2], da[2], db[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        xa[i] = xq[q][0][i]; da[i] = *reinterpret_cast<const float4*>(ca + c);
        xb[i] = xq[q][1][i]; db[i] = *reinterpret_cast<const float4*>(cb + c);
      }
      if (residual) {                                 // dy = A.B^T + residual, the add of the plain GEMM's epilogue
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const float4 ta = rq[q][0][i], tb = rq[q][1][i];
          da[i].x += ta.x; da[i].y += ta.y; da[i].z += ta.z; da[i].w += ta.w;
          db[i].x += tb.x; db[i].y += tb.y; db[i].z += tb.z; db[i].w += tb.w;
        }
      }
      const float ma = mean_in[r0], ra = rstd_in[r0], mb = mean_in[r1], rb = rstd_in[r1];
      float s1a, s2a, s1b, s2b;
      ln_bwd_rows_stats<2>(xa, xb, da, db, gm, dg, ma, ra, mb, rb, two, inv_cols, s1a, s2a, s1b, s2b);
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int c = (lane + 64 * i) * 4;
        float4 o = ln_bwd_row_dx(da[i], xa[i], ra, s1a, s2a);
        st4(dx + r0 * lddx + c, o);
        st4b(dx_bf16 + r0 * ld_bf16 + c, o);
        if (two) {
          o = ln_bwd_row_dx(db[i], xb[i], rb, s1b, s2b);
          st4(dx + r1 * lddx + c, o);
          st4b(dx_bf16 + r1 * ld_bf16 + c, o);
        }
      }
    }
  }
  // block reduction of the dgamma partials through LDS, then one atomic per column and workgroup
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; i++) *reinterpret_cast<float4*>(cs + wave * ROWS_N + (lane + 64 * i) * 4) = dg[i];
  __syncthreads();
  float t = cs[tid];
#pragma unroll
  for (int w = 1; w < 8; w++) t += cs[w * ROWS_N + tid];
  if (t != 0.f) atomicAdd(dgamma + tid, t);
}

// (the entry points of these kernels: end of file, after the weight-gradient kernels)

// =====================================================================================================
// weight gradient:  C[N,K] += A[R,N]^T · B[R,K]
// (the operand images and their swizzle, the zero block, the transposed fragment reads, the k-step of the 64-row kernels and the
// store of a wave's block: gemm_tile.h)
// =====================================================================================================
// DET (all four weight-gradient kernels): the deterministic forms' epilogue.  C is then the caller's scratch with ldc = K and
// every row split STORES its partial tile into slot split_id (C + split_id * N * ldc) instead of adding it into C atomically;
// det_reduce_kernel (elementwise.hip) adds the slots in ascending order.  DET = false is the code it always was.
template <bool DET>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const u16* __restrict__ A, int64_t lda,
                                                       const u16* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                       int64_t ldc, int R, int N, int K, int tiles_k, int rows_per_split, int dbg) {
  __shared__ __attribute__((aligned(16))) u16 lds[2 * 2 * BR * 128];    // 64 KiB
  u16* As = lds;
  u16* Bs = lds + 2 * BR * 128;
  const int tn = blockIdx.x / tiles_k, tk = blockIdx.x % tiles_k;
  const int n0 = tn * 128, k0 = tk * 128;
  const int r_begin = blockIdx.y * rows_per_split;
  int r_end = r_begin + rows_per_split; if (r_end > R) r_end = R;
  if (r_begin >= r_end) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;

  // direct global->LDS staging: the tile image is 64 rows x 16 chunks (1024 chunks) per operand, 4 wave-instructions
  // per wave, A and B in turn
  tn_operand_image<4, 16, 4> ia, ib;
  ia.set(A, n0, N, wave, lane);
  ib.set(B, k0, K, wave, lane);
  auto stage = [&](int r0, int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      ia.load(i, r0, r_end, lda, As + buf * BR * 128, wave);
      ib.load(i, r0, r_end, ldb, Bs + buf * BR * 128, wave);
    }
  };
  f32x16 acc[2][2];
  acc_clear(acc);

  // fragment byte address of (ks, t, i): base[i] + buf*16384 + ks*4096 + t*1024
  const unsigned lds0 = lds_addr(lds), ldsb = lds0 + 2u * 2 * BR * 128;
  const unsigned abase[2] = {tn_frag_base<128>(lds0, wn * 64, lane), tn_frag_base<128>(lds0, wn * 64 + 32, lane)};
  const unsigned bbase[2] = {tn_frag_base<128>(ldsb, wk * 64, lane), tn_frag_base<128>(ldsb, wk * 64 + 32, lane)};
  const int nsteps = (r_end - r_begin + BR - 1) / BR;
  stage(r_begin, 0);
  __syncthreads();
  for (int st = 0; st < nsteps; st++) {
    const int cur = st & 1;
    if (st + 1 < nsteps) stage(r_begin + (st + 1) * BR, cur ^ 1);
    tn_compute_step<4096, 1024>(abase[0] + cur * 16384u, abase[1] + cur * 16384u, bbase[0] + cur * 16384u, bbase[1] + cur * 16384u, acc);
    __syncthreads();
  }
  if (DET) {
    tn_store_tile<true, 2>(acc, C + (int64_t)blockIdx.y * N * ldc, ldc, N, K, n0 + wn * 64, k0 + wk * 64, lane);
  } else if (!(dbg & 1)) {
    tn_store_tile<false, 2>(acc, C, ldc, N, K, n0 + wn * 64, k0 + wk * 64, lane);
  } else {          // dbg & 1 (knob 2, timing ablation): no atomics; the compare keeps the accumulators alive
#pragma unroll
    for (int j = 0; j < 2; j++) {
      if (k0 + wk * 64 + j * 32 + (lane & 31) >= K) continue;
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (acc[i][j][r] == 123.456f) C[0] = 1.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// weight gradient, large variant: 256(n) x 128(k) output tile, 8 wavefronts (4x2, 64x64 each), three LDS stages of
// [64 r][256 n] + [64 r][128 k] (144 KiB) filled by global_load_lds two steps ahead, one raw s_barrier per step with a
// counted vmcnt (same pipeline as gemm_nt_256_kernel), transposed fragment reads in inline asm.
// ---------------------------------------------------------------------------------------------------------
template <bool DET>
__global__ __launch_bounds__(512) void gemm_tn_256_kernel(const u16* __restrict__ A, int64_t lda,
                                                           const u16* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                           int64_t ldc, int R, int N, int K, int tiles_k, int rows_per_split, int dbg) {
  extern __shared__ __attribute__((aligned(16))) u16 ldst[];
  constexpr int STAGE = BR * (256 + 128);        // elements per stage
  // XCD-aware order: the output tiles of ONE row split read the same rows of A and B, so they must share an L2.  The
  // linear workgroup id (XCD = id % 8) is remapped so that each XCD owns a contiguous range of (split, tile) pairs;
  // in launch order the tiles of a split were dealt round the eight XCDs and every XCD fetched every row (PMC: 905 MB
  // fetched per launch against ~330 MB of operands; 318 MB with the remap).
  const int lin0 = (int)(blockIdx.x + gridDim.x * blockIdx.y);
  const int lin = (dbg & 16) ? lin0 : xcd_remap(lin0, (int)(gridDim.x * gridDim.y));          // knob 9 = 16: launch order (A/B)
  const int tile_id = lin % (int)gridDim.x, split_id = lin / (int)gridDim.x;
  const int tn = tile_id / tiles_k, tk = tile_id % tiles_k;
  const int n0 = tn * 256, k0 = tk * 128;
  const int r_begin = split_id * rows_per_split;
  int r_end = r_begin + rows_per_split; if (r_end > R) r_end = R;
  if (r_begin >= r_end) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;

  tn_operand_image<4, 32, 8> ia;          // [64 r][256 n]
  tn_operand_image<2, 16, 8> ib;          // [64 r][128 k]
  ia.set(A, n0, N, wave, lane);
  ib.set(B, k0, K, wave, lane);
  auto stage = [&](int r0, int st) {
    u16* base = ldst + st * STAGE;
#pragma unroll
    for (int i = 0; i < 4; i++) ia.load(i, r0, r_end, lda, base, wave);
#pragma unroll
    for (int i = 0; i < 2; i++) ib.load(i, r0, r_end, ldb, base + BR * 256, wave);
  };
  f32x16 acc[2][2];
  acc_clear(acc);

  const unsigned lds0 = lds_addr(ldst), ldsb = lds0 + 2u * (unsigned)(BR * 256);
  const unsigned abase[2] = {tn_frag_base<256>(lds0, wn * 64, lane), tn_frag_base<256>(lds0, wn * 64 + 32, lane)};
  const unsigned bbase[2] = {tn_frag_base<128>(ldsb, wk * 64, lane), tn_frag_base<128>(ldsb, wk * 64 + 32, lane)};
  const int nsteps = (r_end - r_begin + BR - 1) / BR;
  stage(r_begin, 0);
  if (nsteps > 1) stage(r_begin + BR, 1);
  int st = 0;
  for (int sp = 0; sp < nsteps; sp++) {
    if (sp + 1 < nsteps) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (sp + 2 < nsteps) { int s2 = st + 2; if (s2 >= 3) s2 -= 3; stage(r_begin + (sp + 2) * BR, s2); }
    const unsigned so = (unsigned)st * (unsigned)(STAGE * 2);
    tn_compute_step<8192, 2048>(abase[0] + so, abase[1] + so, bbase[0] + so, bbase[1] + so, acc);
    st = st == 2 ? 0 : st + 1;
  }
  // split_id: the LOGICAL split (after xcd_remap)
  tn_store_tile<DET, 2>(acc, DET ? C + (int64_t)split_id * N * ldc : C, ldc, N, K, n0 + wn * 64, k0 + wk * 64, lane);
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient, 256(n) x 256(k) output tile: the k-loop of these GEMMs is bound by the L2 -> LDS path per CU
// (DESIGN.md section 5), so the lever is bytes per flop: 32 KiB of operands per 32-row step feed 16 MFMAs per
// wavefront, against 24 KiB for the same 16 MFMAs... per 2x the flops: 256x256 moves 2/3 of the bytes per flop of
// 256x128.  8 wavefronts as 4 (n) x 2 (k), each 64 x 128 = 2 x 4 accumulators (128 VGPRs); FIVE LDS stages of
// 32 rows (160 KiB), DMA four steps ahead; fragments by ds_read_b64_tr_b16 (12 per k16-step for 8 MFMAs).
// ---------------------------------------------------------------------------------------------------------
template <bool DET>          // DET: C is this (tile, split) cell's slot, stored; else the gradient, added atomically
__device__ __forceinline__ void tn_256x256_tile(const u16* __restrict__ A, int64_t lda, const u16* __restrict__ B, int64_t ldb,
                                                float* __restrict__ C, int64_t ldc, int N, int K, int tn, int tk, int r_begin,
                                                int r_end, u16* ldst) {
  const int n0 = tn * 256, k0 = tk * 256;
  if (r_begin >= r_end) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const u16* zero = reinterpret_cast<const u16*>(g_zero16);

  // DMA: an operand image is 1024 chunks of 16 B = 16 wave-instructions, two per wave; position p -> row p >> 5, chunk
  // position p & 31 holds logical chunk (p & 31) ^ ((row & 3) << 2).  Every lane keeps a running source pointer per load (rows
  // advance by 32 per stage), so a stage whose 32 rows all exist
  // costs four loads and four 64-bit adds; only a split's last, partial stage tests rows.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  int srow[2];
  const u16* cur_a[2];
  const u16* cur_b[2];
  const int64_t inc_a = (int64_t)BR2 * lda, inc_b = (int64_t)BR2 * ldb;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int p = (i * 8 + wave) * 64 + lane, r = p >> 5, c = (p & 31) ^ ((r & 3) << 2);
    srow[i] = r;
    // a column block past the matrix re-reads the last one inside it: those products land in rows / columns of C that are not stored
    int ca = n0 + c * 8, cb = k0 + c * 8;
    if (ca >= N) ca = (N - 1) & ~7;
    if (cb >= K) cb = (K - 1) & ~7;
    cur_a[i] = A + ca + (int64_t)(r_begin + r) * lda;
    cur_b[i] = B + cb + (int64_t)(r_begin + r) * ldb;
  }
  int r_next = r_begin;          // first row of the next stage to be issued (stages are issued in row order)
  auto stage = [&](int st) {
    u16* base = ldst + st * TN2_STAGE;
    const bool whole = r_next + BR2 <= r_end;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const bool in = whole || r_next + srow[i] < r_end;
      // (the builtin spelled out, not lds_dma16: through the wrapper the compiler reordered this block of the k-loop - m0 writes,
      //  selects, loads - and the grouped launch measured 2 % slower)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? cur_a[i] : zero),
                                       (__attribute__((address_space(3))) void*)(base + (i * 8 + wave_u) * 512), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(in ? cur_b[i] : zero),
                                       (__attribute__((address_space(3))) void*)(base + BR2 * 256 + (i * 8 + wave_u) * 512), 16, 0, 0);
      cur_a[i] += inc_a; cur_b[i] += inc_b;
    }
    r_next += BR2;
  };
  // (its own loop, not acc_clear: with the call the grouped kernel's registers came out differently - the listing loses the s_nop in
  //  front of the k-step's first MFMA - and the grouped launch measured 2 % slower, profiles/gemm_tile_isa.md)
  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

  // transposed reads (tn_frag_base): + 4 rows for read t = 1, + 16 rows per k16-step
  const unsigned lds0 = lds_addr(ldst), ldsb = lds0 + 2u * (unsigned)(BR2 * 256);
  const unsigned abase[2] = {tn_frag_base<256>(lds0, wn * 64, lane), tn_frag_base<256>(lds0, wn * 64 + 32, lane)};
  unsigned bbase[4];
#pragma unroll
  for (int j = 0; j < 4; j++) bbase[j] = tn_frag_base<256>(ldsb, wk * 128 + j * 32, lane);
  // FIVE stages of 32 rows (all 160 KiB of LDS), DMA four steps ahead.  The step is the software-pipelined one of gemm_tile.h
  // (T256_GROUP_READING): a block's two transposed reads per MFMA gap, the step's one barrier between its two MFMA groups, and one
  // MFMA before the next stage's DMA is issued.
  const int nsteps = (r_end - r_begin + BR2 - 1) / BR2;
  stage(0);
  if (nsteps > 1) stage(1);
  if (nsteps > 2) stage(2);
  if (nsteps > 3) stage(3);
  u32x2v fa[2][2][2], fb[2][4][2];          // [k16-step][block][t]
#define TN2_RA(KS, I, SO) TR_READ(fa[KS][I][0], abase[I] + (SO), (KS) * 8192); TR_READ(fa[KS][I][1], abase[I] + (SO), (KS) * 8192 + 2048); T256_SB
#define TN2_RB(KS, J, SO) TR_READ(fb[KS][J][0], bbase[J] + (SO), (KS) * 8192); TR_READ(fb[KS][J][1], bbase[J] + (SO), (KS) * 8192 + 2048); T256_SB
#define TN2_AF(KS, I) __builtin_bit_cast(bf16x8, make_uint4(fa[KS][I][0][0], fa[KS][I][0][1], fa[KS][I][1][0], fa[KS][I][1][1]))
#define TN2_BF(KS, J) __builtin_bit_cast(bf16x8, make_uint4(fb[KS][J][0][0], fb[KS][J][0][1], fb[KS][J][1][0], fb[KS][J][1][1]))
#define TN2_MM(KS, I, J) acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TN2_AF(KS, I), TN2_BF(KS, J), acc[I][J], 0, 0, 0); T256_SB
#define TN2_GROUP_READING(KS, KN, SO, MID) T256_GROUP_READING(TN2_RA, TN2_RB, TN2_MM, KS, KN, SO, MID)
  if (nsteps > 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (nsteps > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (nsteps > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  T256_SB
  T256_FIRST_READS(TN2_RA, TN2_RB)
  int st = 0, prev = TN2_NSTAGE - 1;
  for (int sp = 0; sp + 1 < nsteps; sp++) {
    const unsigned so = (unsigned)st * (unsigned)(TN2_STAGE * 2);
    const int nxt = st == TN2_NSTAGE - 1 ? 0 : st + 1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    TN2_GROUP_READING(0, 1, so, )
    // stage sp + 1 has landed once only the (4 loads each of the) two younger stages are outstanding; past the barrier every
    // wavefront has finished with stage sp - 1, whose buffer takes stage sp + 4
    if (sp + 3 < nsteps) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
    else if (sp + 2 < nsteps) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    T256_SB
    const unsigned son = (unsigned)nxt * (unsigned)(TN2_STAGE * 2);
    const bool fetch = sp + 4 < nsteps;
    TN2_GROUP_READING(1, 0, son, if (fetch) stage(prev); T256_SB)
    prev = st; st = nxt;
  }
  {          // the last stage: nothing left to wait for or to fetch
    const unsigned so = (unsigned)st * (unsigned)(TN2_STAGE * 2);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    TN2_GROUP_READING(0, 1, so, )
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); T256_SB
    T256_GROUP(TN2_MM, 1)
  }
#undef TN2_RA
#undef TN2_RB
#undef TN2_AF
#undef TN2_BF
#undef TN2_MM
#undef TN2_GROUP_READING
  tn_store_tile<DET, 4>(acc, C, ldc, N, K, n0 + wn * 64, k0 + wk * 128, lane);
}

template <bool DET>
__global__ __launch_bounds__(512) void gemm_tn_256x256_kernel(const u16* __restrict__ A, int64_t lda,
                                                               const u16* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                               int64_t ldc, int R, int N, int K, int tiles_k, int rows_per_split, int dbg) {
  extern __shared__ __attribute__((aligned(16))) u16 ldst[];
  const int lin0 = (int)(blockIdx.x + gridDim.x * blockIdx.y);
  const int lin = (dbg & 16) ? lin0 : xcd_remap(lin0, (int)(gridDim.x * gridDim.y));          // tiles of one split on one XCD
  const int tile_id = lin % (int)gridDim.x, split_id = lin / (int)gridDim.x;
  const int r_begin = split_id * rows_per_split;
  int r_end = r_begin + rows_per_split; if (r_end > R) r_end = R;
  tn_256x256_tile<DET>(A, lda, B, ldb, DET ? C + (int64_t)split_id * N * ldc : C, ldc, N, K, tile_id / tiles_k, tile_id % tiles_k, r_begin, r_end, ldst);
}

// Several weight gradients over the SAME token rows in one launch (the four of a transformer layer): the launch then has
// 48 tiles instead of 12, so a full round of workgroups needs 5 row splits instead of 21 and the fp32 atomic traffic (every
// split adds the whole gradient once; a quarter to a third of the single launches' time) drops four-fold.
struct tn_group {
  const u16* A[MCA_TN_MAX_GROUP];
  const u16* B[MCA_TN_MAX_GROUP];
  float* C[MCA_TN_MAX_GROUP];
  int64_t lda[MCA_TN_MAX_GROUP], ldb[MCA_TN_MAX_GROUP], ldc[MCA_TN_MAX_GROUP];
  int N[MCA_TN_MAX_GROUP], K[MCA_TN_MAX_GROUP], tiles_k[MCA_TN_MAX_GROUP];
  int first_tile[MCA_TN_MAX_GROUP + 1];
  int n, R, tiles;
  int unit, n_full, span;          // the balanced row partition: mca_tn_partition (gemm_plan.h), planned by mca_plan_gemm_tn_group
  int own;
};
// DET: the uniform partition only (n_full splits, no line: every workgroup is one (tile, split) cell); g.C[p] / g.ldc[p] are member
// p's place in slot 0 of the scratch; a slot is the members' packed partials one after the other
template <bool DET>
__global__ __launch_bounds__(512) void gemm_tn_256x256_group_kernel(tn_group g, int dbg) {
  extern __shared__ __attribute__((aligned(16))) u16 ldst[];
  const int lin0 = (int)blockIdx.x;
  const int lin = (dbg & 16) ? lin0 : xcd_remap(lin0, (int)gridDim.x);          // tiles of one split on one XCD
#ifdef MCA_TRACE_BUILD          // clock probe (knob 9 bit 8): shader cycles and 100 MHz ticks of every workgroup's lifetime (tools/ablate_tn_group.py)
  const bool probe = (dbg & 8) && threadIdx.x == 0 && lin0 < 512;
  const uint64_t c0 = probe ? __builtin_amdgcn_s_memtime() : 0, t0 = probe ? __builtin_amdgcn_s_memrealtime() : 0;
#endif
  // (the segment arithmetic below has a line-for-line host copy, mca_tn_group_segments in gemm_plan.h, which the CPU tests run:
  //  change both or neither)
  const int n_cells = g.n_full * g.tiles;
  const int row0 = g.n_full * g.unit, rest = g.R - row0;          // rows [row0, R) of every tile
  // this workgroup's span [s, e) of the tile-major line over tiles line0 .. tiles - 1 (a whole cell is the degenerate case: one
  // segment, no line arithmetic)
  const int line0 = g.own;
  int64_t s = 0, e = 0;
  bool own_pending = false;
  if (lin >= n_cells) {
    const int j = lin - n_cells;
    own_pending = j < g.own;
    s = (int64_t)j * g.span;
    e = s + g.span;
    const int64_t line = (int64_t)(g.tiles - line0) * rest;
    if (e > line) e = line;
  }
  int64_t slot_stride = 0;          // floats from one split's slot to the next
  if constexpr (DET) {
#pragma unroll
    for (int i = 0; i < MCA_TN_MAX_GROUP; i++) if (i < g.n) slot_stride += (int64_t)g.N[i] * g.K[i];
  }
  bool first = true;
  for (;;) {
    int tile_all, r_begin, r_end;
    if (lin < n_cells) {
      tile_all = lin % g.tiles;
      r_begin = (lin / g.tiles) * g.unit; r_end = r_begin + g.unit;
    } else if (own_pending) {
      own_pending = false;
      tile_all = lin - n_cells;
      r_begin = row0; r_end = g.R;
    } else {
      if (s >= e) break;
      const int t = (int)(s / rest);
      tile_all = line0 + t;
      const int off = (int)(s - (int64_t)t * rest);
      int len = rest - off; if ((int64_t)len > e - s) len = (int)(e - s);
      r_begin = row0 + off; r_end = r_begin + len;
      s += len;
    }
    if (r_end > g.R) r_end = g.R;
    int p = 0;
#pragma unroll
    for (int i = 1; i < MCA_TN_MAX_GROUP; i++) if (i < g.n && tile_all >= g.first_tile[i]) p = i;
    const int tile_id = tile_all - g.first_tile[p];
    if (!first) __syncthreads();          // the previous segment's last fragment reads, before this one's DMA lands in the ring
    first = false;
    tn_256x256_tile<DET>(g.A[p], g.lda[p], g.B[p], g.ldb[p], DET ? g.C[p] + (int64_t)(lin / g.tiles) * slot_stride : g.C[p], g.ldc[p], g.N[p], g.K[p],
                         tile_id / g.tiles_k[p], tile_id % g.tiles_k[p], r_begin, r_end, ldst);
    if (lin < n_cells) break;
  }
#ifdef MCA_TRACE_BUILD
  if (probe) { mca_trace_gemm[2 * lin0] = __builtin_amdgcn_s_memtime() - c0; mca_trace_gemm[2 * lin0 + 1] = __builtin_amdgcn_s_memrealtime() - t0; }
#endif
}

// =====================================================================================================
// Entry points: validate, plan (gemm_plan.h), launch what the plan says.
// =====================================================================================================
struct gemm_operands {
  const u16* A; int64_t lda;
  const u16* B; int64_t ldb;
  void* C; int64_t ldc;
  const float* bias;
  const float* residual; int64_t ldres, res_period;          // the GEGLU fusions pass h (backward) / g (forward) here
  const float *ln_mean, *ln_rstd, *ln_gamma;
  int M, K;                                                  // (weight gradient: M = R, the rows reduced)
  const tn_group* group;
};

template <auto KERNEL, typename... Args>
static int launch_kernel(const mca_gemm_plan& p, mca_stream_t stream, Args... args) {
  if (p.lds_bytes && !mca_dyn_lds<KERNEL>(p.lds_bytes)) return MCA_E_LAUNCH;
  hipLaunchKernelGGL(KERNEL, dim3(p.grid_x, p.grid_y), dim3(p.block), p.lds_bytes, as_stream(stream), args...);
  return launch_status();
}
// the four argument lists of the NT kernels, and the weight gradient's
template <bool OB, int RS, int EPI>
static int launch_glds(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  return launch_kernel<gemm_nt_glds_kernel<OB, RS, 64, EPI>>(p, s, o.A, o.lda, o.B, o.ldb, o.C, o.ldc, o.bias, o.residual, o.ldres, o.res_period,
                                                             o.M, p.n, o.K, p.tiles_n, p.nwg);
}
template <bool OB, int RS, int PF, int EPI>
static int launch_256(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  return launch_kernel<gemm_nt_256_kernel<OB, RS, PF, EPI>>(p, s, o.A, o.lda, o.B, o.ldb, o.C, o.ldc, o.bias, o.residual, o.ldres, o.res_period,
                                                            o.M, p.n, o.K, p.tiles_n, p.nwg, o.ln_mean, o.ln_rstd, o.ln_gamma);
}
template <int MODE, bool BIAS>
static int launch_persist(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  return launch_kernel<gemm_nt_persist_kernel<MODE, BIAS>>(p, s, o.A, o.lda, o.B, o.ldb, o.C, o.ldc, o.bias, o.residual, o.ldres, o.M, p.n, o.K,
                                                           p.tiles_n, p.nwg, p.dbg);
}
template <bool GEGLU, bool SAVED = false, bool CB = false>          // CB: o.ldc is the slab stride cbs
static int launch_persist256(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  u16* g = GEGLU ? reinterpret_cast<u16*>(const_cast<float*>(o.residual)) : nullptr;
  return launch_kernel<gemm_nt_persist256_kernel<GEGLU, SAVED, CB>>(p, s, o.A, o.lda, o.B, o.ldb, reinterpret_cast<u16*>(o.C), o.ldc, g,
                                                         GEGLU ? o.ldres : (int64_t)0, o.M, p.n, o.K, p.tiles_n, p.nwg, p.dbg);
}
template <auto KERNEL>
static int launch_tn(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  return launch_kernel<KERNEL>(p, s, o.A, o.lda, o.B, o.ldb, reinterpret_cast<float*>(o.C), o.ldc, o.M, p.n, o.K, p.tiles_k, p.rows_per_split, p.dbg);
}

static int launch(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  switch (p.kernel) {
    case MCA_GK_NT_GLDS + 0: return launch_glds<false, 0, 0>(p, o, s);
    case MCA_GK_NT_GLDS + 1: return launch_glds<false, 1, 0>(p, o, s);
    case MCA_GK_NT_GLDS + 2: return launch_glds<false, 2, 0>(p, o, s);
    case MCA_GK_NT_GLDS + 3: return launch_glds<true, 0, 0>(p, o, s);
    case MCA_GK_NT_GLDS + 4: return launch_glds<true, 1, 0>(p, o, s);
    case MCA_GK_NT_GLDS + 5: return launch_glds<true, 2, 0>(p, o, s);
    case MCA_GK_NT_GLDS_GEGLU_BWD: return launch_glds<true, 0, 1>(p, o, s);
    case MCA_GK_NT_256 + 0: return launch_256<false, 0, 0, 0>(p, o, s);
    case MCA_GK_NT_256 + 1: return launch_256<false, 1, 0, 0>(p, o, s);
    case MCA_GK_NT_256 + 2: return launch_256<false, 2, 0, 0>(p, o, s);
    case MCA_GK_NT_256 + 3: return launch_256<true, 0, 0, 0>(p, o, s);
    case MCA_GK_NT_256 + 4: return launch_256<true, 1, 0, 0>(p, o, s);
    case MCA_GK_NT_256 + 5: return launch_256<true, 2, 0, 0>(p, o, s);
    case MCA_GK_NT_256_PF: return launch_256<false, 1, 1, 0>(p, o, s);
    case MCA_GK_NT_256_LNRES: return launch_256<false, 1, 1, 2>(p, o, s);
    case MCA_GK_NT_256_GEGLU_BWD: return launch_256<true, 0, 0, 1>(p, o, s);
    case MCA_GK_NT_PERSIST + 0: return launch_persist<0, false>(p, o, s);
    case MCA_GK_NT_PERSIST + 1: return launch_persist<0, true>(p, o, s);
    case MCA_GK_NT_PERSIST + 2: return launch_persist<1, false>(p, o, s);
    case MCA_GK_NT_PERSIST + 3: return launch_persist<1, true>(p, o, s);
    case MCA_GK_NT_PERSIST + 4: return launch_persist<2, false>(p, o, s);
    case MCA_GK_NT_PERSIST + 5: return launch_persist<2, true>(p, o, s);
    case MCA_GK_NT_PERSIST_GEGLU_BWD: return launch_persist<3, false>(p, o, s);
    case MCA_GK_NT_PERSIST_GEGLU_FWD: return launch_persist<4, false>(p, o, s);
    case MCA_GK_NT_PERSIST256: return launch_persist256<false>(p, o, s);
    case MCA_GK_NT_PERSIST256_GEGLU_FWD: return launch_persist256<true>(p, o, s);
    case MCA_GK_NT_GLDS_GEGLU_BWD_SAVED: return launch_glds<true, 0, 3>(p, o, s);
    case MCA_GK_NT_256_GEGLU_BWD_SAVED: return launch_256<true, 0, 0, 3>(p, o, s);
    case MCA_GK_NT_PERSIST_GEGLU_BWD_SAVED: return launch_persist<5, false>(p, o, s);
    case MCA_GK_NT_PERSIST_GEGLU_FWD_SAVED: return launch_persist<6, false>(p, o, s);
    case MCA_GK_NT_PERSIST256_GEGLU_FWD_SAVED: return launch_persist256<true, true>(p, o, s);
    case MCA_GK_NT_PERSIST256_CB: return launch_persist256<false, false, true>(p, o, s);
    case MCA_GK_TN: return launch_tn<gemm_tn_kernel<false>>(p, o, s);
    case MCA_GK_TN_256: return launch_tn<gemm_tn_256_kernel<false>>(p, o, s);
    case MCA_GK_TN_256X256: return launch_tn<gemm_tn_256x256_kernel<false>>(p, o, s);
    case MCA_GK_TN_256X256_GROUP: return launch_kernel<gemm_tn_256x256_group_kernel<false>>(p, s, *o.group, p.dbg);
  }
  return MCA_E_LAUNCH;          // a plan without a kernel is a missing kernel, never a quiet no-op
}
// the deterministic instantiations of the four weight-gradient kernels (o.C: the scratch, o.ldc: K)
static int launch_det(const mca_gemm_plan& p, const gemm_operands& o, mca_stream_t s) {
  switch (p.kernel) {
    case MCA_GK_TN: return launch_tn<gemm_tn_kernel<true>>(p, o, s);
    case MCA_GK_TN_256: return launch_tn<gemm_tn_256_kernel<true>>(p, o, s);
    case MCA_GK_TN_256X256: return launch_tn<gemm_tn_256x256_kernel<true>>(p, o, s);
    case MCA_GK_TN_256X256_GROUP: return launch_kernel<gemm_tn_256x256_group_kernel<true>>(p, s, *o.group, p.dbg);
  }
  return MCA_E_LAUNCH;
}

static uint64_t addr(const void* p) { return (uint64_t)(uintptr_t)p; }

extern "C" int mca_gemm_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc,
                           int out_bf16, const float* bias, const float* residual, int64_t ldres,
                           int64_t res_period, int64_t M, int64_t N, int64_t K, mca_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  if (K % 64 || lda % 8 || ldb % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16) return MCA_E_ALIGN;
  if (lda < K || ldb < K || ldc < N) return MCA_E_BADARG;
  if (M > (1LL << 30) || N > (1LL << 30)) return MCA_E_UNSUPPORTED;
  const mca_nt_problem pr = {M, N, K, out_bf16, res_period, addr(C), addr(bias), addr(residual), ldc, ldres};
  const gemm_operands o = {A, lda, B, ldb, C, ldc, bias, residual, ldres, res_period, nullptr, nullptr, nullptr, (int)M, (int)K, nullptr};
  return launch(mca_plan_gemm_nt(pr, mca_knobs, num_cus()), o, stream);
}

// C = A·B^T (bf16) stored column-blocked, [N / 64][M][64] with cbs elements between the slabs (include/mca_hip.h)
extern "C" int mca_gemm_nt_cb(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t cbs,
                              int64_t M, int64_t N, int64_t K, mca_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  if (K % 32 || lda % 8 || ldb % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16) return MCA_E_ALIGN;
  if (lda < K || ldb < K) return MCA_E_BADARG;
  if (M > (1LL << 30) || N > (1LL << 30)) return MCA_E_UNSUPPORTED;
  mca_gemm_plan pl;
  if (!mca_plan_gemm_nt_cb(M, N, K, addr(C), cbs, mca_knobs, num_cus(), &pl)) return MCA_E_UNSUPPORTED;
  const gemm_operands o = {A, lda, B, ldb, C, cbs, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, (int)M, (int)K, nullptr};
  return launch(pl, o, stream);
}

// C[M,N] (fp32) = A·B^T + LayerNorm(x) with the LayerNorm recomputed in the epilogue from x and its saved statistics.
extern "C" int mca_gemm_nt_lnres(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                                 const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                 int64_t M, int64_t N, int64_t K, mca_stream_t stream) {
  if (!A || !B || !C || !x || !mean || !rstd || !gamma || M <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  if (K % 64 || lda % 8 || ldb % 8 || ldc % 4 || ldx % 4 || (uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)C % 16 ||
      (uintptr_t)x % 16 || (uintptr_t)gamma % 16)
    return MCA_E_ALIGN;
  if (lda < K || ldb < K || ldc < N || ldx < N) return MCA_E_BADARG;
  if (!mca_nt_lnres_supported(M, N, K)) return MCA_E_UNSUPPORTED;
  const gemm_operands o = {A, lda, B, ldb, C, ldc, nullptr, x, ldx, 0, mean, rstd, gamma, (int)M, (int)K, nullptr};
  return launch(mca_plan_gemm_nt_lnres(M, N), o, stream);
}

// LayerNorm backward of dy = A·B^T (+ residual) in the epilogue of the full-row kernel: dy is never written (include/mca_hip.h).
// (what both entry points refuse, in this order, before anything is planned or launched)
static int res_lnbwd_refusal(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual, int64_t ldres,
                             const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                             float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16, float* dgamma, int64_t M, int64_t N, int64_t K) {
  if (!A || !B || !x || !mean || !rstd || !gamma || !dx || !dx_bf16 || !dgamma || M <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  const int refusal = mca_nt_rows_refusal(M, N, K);
  if (refusal) return refusal;
  if (lda % 8 || ldb % 8 || ldx % 4 || lddx % 4 || ld_bf16 % 8 || (residual && ldres % 4) || (uintptr_t)A % 16 || (uintptr_t)B % 16 ||
      (uintptr_t)x % 16 || (uintptr_t)gamma % 16 || (uintptr_t)dx % 16 || (uintptr_t)dx_bf16 % 16 || (uintptr_t)residual % 16)
    return MCA_E_ALIGN;
  if (lda < K || ldb < K || ldx < N || lddx < N || ld_bf16 < N || (residual && ldres < N)) return MCA_E_BADARG;
  return MCA_OK;
}
extern "C" int mca_gemm_nt_res_lnbwd(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual, int64_t ldres,
                                     const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                     float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16, float* dgamma,
                                     int64_t M, int64_t N, int64_t K, mca_stream_t stream) {
  const int rc = res_lnbwd_refusal(A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16, ld_bf16, dgamma, M, N, K);
  if (rc != MCA_OK) return rc;
  const mca_gemm_plan p = mca_plan_gemm_nt_res_lnbwd(M);
  return launch_kernel<gemm_nt_rows_kernel>(p, stream, A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16, ld_bf16,
                                               dgamma, (int)M, (int)K, p.nwg);
}
// The same with the tile height chosen for the device's CU count (mca_nt_rows_height): gemm_nt_rows160_kernel where 160-row tiles
// save a round of workgroups, gemm_nt_rows_kernel and the plan above everywhere else.
extern "C" int mca_gemm_nt_res_lnbwd_tall(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* residual, int64_t ldres,
                                          const float* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                                          float* dx, int64_t lddx, uint16_t* dx_bf16, int64_t ld_bf16, float* dgamma,
                                          int64_t M, int64_t N, int64_t K, mca_stream_t stream) {
  const int rc = res_lnbwd_refusal(A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16, ld_bf16, dgamma, M, N, K);
  if (rc != MCA_OK) return rc;
  const mca_gemm_plan p = mca_plan_gemm_nt_res_lnbwd_tall(M, mca_knobs, num_cus());
  switch (p.kernel) {
    case MCA_GK_NT_ROWS_LNBWD:
      return launch_kernel<gemm_nt_rows_kernel>(p, stream, A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16, ld_bf16,
                                                   dgamma, (int)M, (int)K, p.nwg);
    case MCA_GK_NT_ROWS160_LNBWD:
      return launch_kernel<gemm_nt_rows160_kernel>(p, stream, A, lda, B, ldb, residual, ldres, x, ldx, mean, rstd, gamma, dx, lddx, dx_bf16,
                                                      ld_bf16, dgamma, (int)M, (int)K, p.nwg);
  }
  return MCA_E_LAUNCH;
}

// dh = GEGLU'(h) applied to dg = A·B^T without materialising dg (fused epilogue).  A[M,K] (= d x_out, bf16), B[ip,K] (= W2^T
// copy), h / dh [M, 2*ip] bf16.
// (saved: h holds the forward's saved factors s, include/mca_hip.h)
static int geglu_bwd_entry(bool saved, const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* h,
                           uint16_t* dh, int64_t ldh, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  if (!A || !B || !h || !dh || M <= 0 || ip <= 0 || K <= 0) return MCA_E_BADARG;
  if (K % 64 || lda % 8 || ldb % 8 || ldh % 8 || ip % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16 || (uintptr_t)h % 16 || (uintptr_t)dh % 16)
    return MCA_E_ALIGN;
  if (lda < K || ldb < K || ldh < 2 * ip) return MCA_E_BADARG;
  if (M > (1LL << 30)) return MCA_E_UNSUPPORTED;
  const gemm_operands o = {A, lda, B, ldb, dh, ldh, nullptr, reinterpret_cast<const float*>(h), ldh, 0, nullptr, nullptr, nullptr, (int)M, (int)K, nullptr};
  return launch(saved ? mca_plan_gemm_nt_geglu_bwd_saved(M, ip, K, mca_knobs, num_cus()) : mca_plan_gemm_nt_geglu_bwd(M, ip, K, mca_knobs, num_cus()),
                o, stream);
}
extern "C" int mca_gemm_nt_geglu_bwd(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* h,
                                     uint16_t* dh, int64_t ldh, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  return geglu_bwd_entry(false, A, lda, B, ldb, h, dh, ldh, ip, M, K, stream);
}
extern "C" int mca_gemm_nt_geglu_bwd_saved(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const uint16_t* s,
                                           uint16_t* dh, int64_t ldh, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  return geglu_bwd_entry(true, A, lda, B, ldb, s, dh, ldh, ip, M, K, stream);
}

// h = A·W1^T (bf16, [a | gate]) and g = a * gelu(gate) in one pass (persistent kernels); small or oddly shaped
// problems take the plain GEMM followed by the element-wise kernel.
// (saved: h receives the saved factors s instead, include/mca_hip.h)
static int geglu_fwd_entry(bool saved, const uint16_t* A, int64_t lda, const uint16_t* W1, int64_t ldb, uint16_t* h, int64_t ldh,
                           uint16_t* g, int64_t ldg, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  if (!A || !W1 || !h || !g || M <= 0 || ip <= 0 || K <= 0) return MCA_E_BADARG;
  if (K % 64 || lda % 8 || ldb % 8 || ldh % 8 || ldg % 8 || ip % 8 || (uintptr_t)A % 16 || (uintptr_t)W1 % 16 || (uintptr_t)h % 16 ||
      (uintptr_t)g % 16)
    return MCA_E_ALIGN;
  if (lda < K || ldb < K || ldh < 2 * ip || ldg < ip) return MCA_E_BADARG;
  if (M > (1LL << 30)) return MCA_E_UNSUPPORTED;
  const mca_gemm_plan p = saved ? mca_plan_gemm_nt_geglu_fwd_saved(M, ip, K, mca_knobs, num_cus()) : mca_plan_gemm_nt_geglu_fwd(M, ip, K, mca_knobs, num_cus());
  if (p.kernel != MCA_GK_NONE) {
    const gemm_operands o = {A, lda, W1, ldb, h, ldh, nullptr, reinterpret_cast<const float*>(g), ldg, 0, nullptr, nullptr, nullptr, (int)M, (int)K, nullptr};
    return launch(p, o, stream);
  }
  if (ldg != ip || ldh != 2 * ip) return MCA_E_UNSUPPORTED;          // the element-wise kernel takes packed rows
  const int rc = mca_gemm_nt(A, lda, W1, ldb, h, ldh, 1, nullptr, nullptr, 0, 0, M, 2 * ip, K, stream);
  if (rc != MCA_OK) return rc;
  return saved ? mca_geglu_fwd_saved(h, g, M, (int)ip, stream) : mca_geglu_fwd(h, g, M, (int)ip, stream);
}
extern "C" int mca_gemm_nt_geglu_fwd(const uint16_t* A, int64_t lda, const uint16_t* W1, int64_t ldb, uint16_t* h, int64_t ldh,
                                     uint16_t* g, int64_t ldg, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  return geglu_fwd_entry(false, A, lda, W1, ldb, h, ldh, g, ldg, ip, M, K, stream);
}
extern "C" int mca_gemm_nt_geglu_fwd_saved(const uint16_t* A, int64_t lda, const uint16_t* W1, int64_t ldb, uint16_t* s, int64_t lds,
                                           uint16_t* g, int64_t ldg, int64_t ip, int64_t M, int64_t K, mca_stream_t stream) {
  return geglu_fwd_entry(true, A, lda, W1, ldb, s, lds, g, ldg, ip, M, K, stream);
}

static int check_tn(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, const float* C, int64_t ldc, int64_t N, int64_t K) {
  if (!A || !B || !C || N <= 0 || K <= 0) return MCA_E_BADARG;
  if (lda % 8 || ldb % 8 || (uintptr_t)A % 16 || (uintptr_t)B % 16) return MCA_E_ALIGN;
  if (lda < (N + 7) / 8 * 8 || ldb < (K + 7) / 8 * 8 || ldc < K) return MCA_E_BADARG;
  return MCA_OK;
}

extern "C" int mca_gemm_tn_acc(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                               int64_t R, int64_t N, int64_t K, mca_stream_t stream) {
  if (R <= 0) return MCA_E_BADARG;
  const int rc = check_tn(A, lda, B, ldb, C, ldc, N, K);
  if (rc != MCA_OK) return rc;
  if (R > (1LL << 30)) return MCA_E_UNSUPPORTED;
  const gemm_operands o = {A, lda, B, ldb, C, ldc, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, (int)R, (int)K, nullptr};
  return launch(mca_plan_gemm_tn(R, N, K, mca_knobs), o, stream);
}

extern "C" int mca_gemm_tn_acc_group(const mca_tn_desc* d, int n, int64_t R, mca_stream_t stream) {
  if (!d || n <= 0 || n > MCA_TN_MAX_GROUP || R <= 0) return MCA_E_BADARG;
  if (R > (1LL << 30)) return MCA_E_UNSUPPORTED;
  tn_group g;
  int tiles = 0;
  bool all_taken = true;
  for (int i = 0; i < n; i++) {
    const int rc = check_tn(d[i].A, d[i].lda, d[i].B, d[i].ldb, d[i].C, d[i].ldc, d[i].N, d[i].K);
    if (rc != MCA_OK) return rc;
    const int t = mca_tn_group_member_tiles(d[i].N, d[i].K);
    all_taken = all_taken && t > 0;
    g.A[i] = d[i].A; g.B[i] = d[i].B; g.C[i] = d[i].C;
    g.lda[i] = d[i].lda; g.ldb[i] = d[i].ldb; g.ldc[i] = d[i].ldc;
    g.N[i] = (int)d[i].N; g.K[i] = (int)d[i].K;
    g.tiles_k[i] = (int)((d[i].K + 255) / 256);
    g.first_tile[i] = tiles;
    tiles += t;
  }
  const mca_tn_group_plan p = mca_plan_gemm_tn_group(all_taken ? tiles : 0, n, R, mca_knobs, num_cus());
  if (p.grouped < 0) return p.grouped;
  if (!p.grouped) {          // members the grouped kernel does not suit, or a group too small to fill the chip: one launch each
    for (int i = 0; i < n; i++) {
      const int rc = mca_gemm_tn_acc(d[i].A, d[i].lda, d[i].B, d[i].ldb, d[i].C, d[i].ldc, R, d[i].N, d[i].K, stream);
      if (rc != MCA_OK) return rc;
    }
    return MCA_OK;
  }
  for (int i = n; i <= MCA_TN_MAX_GROUP; i++) g.first_tile[i] = tiles;
  g.n = n; g.R = p.part.R; g.tiles = p.part.tiles;
  g.unit = p.part.unit; g.n_full = p.part.n_full; g.span = p.part.span; g.own = p.part.own;
  gemm_operands o = {};
  o.group = &g;
  return launch(p.launch, o, stream);
}

// ---- deterministic forms (include/mca_hip.h, "Deterministic mode"): partial slabs into the caller's scratch, then the ordered reduce
extern "C" int64_t mca_gemm_tn_acc_det_scratch(int64_t R, int64_t N, int64_t K) {
  if (R <= 0 || N <= 0 || K <= 0 || R > (1LL << 30)) return 0;
  return mca_plan_gemm_tn_det(R, N, K, mca_knobs).scratch_floats;
}
extern "C" int64_t mca_gemm_tn_acc_group_det_scratch(const int64_t* N, const int64_t* K, int n, int64_t R, int cus) {
  if (!N || !K || n <= 0 || n > MCA_TN_MAX_GROUP || R <= 0 || R > (1LL << 30)) return 0;
  return mca_plan_gemm_tn_group_det(N, K, n, R, mca_knobs, cus > 0 ? cus : num_cus()).scratch_floats;
}

extern "C" int mca_gemm_tn_acc_det(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                                   int64_t R, int64_t N, int64_t K, float* scratch, int64_t scratch_floats, mca_stream_t stream) {
  if (R <= 0) return MCA_E_BADARG;
  int rc = check_tn(A, lda, B, ldb, C, ldc, N, K);
  if (rc != MCA_OK) return rc;
  if (R > (1LL << 30)) return MCA_E_UNSUPPORTED;
  const mca_tn_det_plan p = mca_plan_gemm_tn_det(R, N, K, mca_knobs);
  if (p.slots <= 1) return mca_gemm_tn_acc(A, lda, B, ldb, C, ldc, R, N, K, stream);          // one contributor per element
  if (!scratch || scratch_floats < p.scratch_floats) return MCA_E_BADARG;
  const gemm_operands o = {A, lda, B, ldb, scratch, K, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, (int)R, (int)K, nullptr};
  rc = launch_det(p.launch, o, stream);
  if (rc != MCA_OK) return rc;
  return mca_det_reduce(scratch, p.slot_stride, p.slots, C, ldc, N, (int)K, stream);
}

extern "C" int mca_gemm_tn_acc_group_det(const mca_tn_desc* d, int n, int64_t R, float* scratch, int64_t scratch_floats, mca_stream_t stream) {
  if (!d || n <= 0 || n > MCA_TN_MAX_GROUP || R <= 0) return MCA_E_BADARG;
  if (R > (1LL << 30)) return MCA_E_UNSUPPORTED;
  int64_t Ns[MCA_TN_MAX_GROUP], Ks[MCA_TN_MAX_GROUP];
  for (int i = 0; i < n; i++) {
    const int rc = check_tn(d[i].A, d[i].lda, d[i].B, d[i].ldb, d[i].C, d[i].ldc, d[i].N, d[i].K);
    if (rc != MCA_OK) return rc;
    Ns[i] = d[i].N; Ks[i] = d[i].K;
  }
  const mca_tn_group_det_plan p = mca_plan_gemm_tn_group_det(Ns, Ks, n, R, mca_knobs, num_cus());
  if (p.plan.grouped < 0) return p.plan.grouped;
  if (p.scratch_floats > 0 && (!scratch || scratch_floats < p.scratch_floats)) return MCA_E_BADARG;          // before anything is launched
  if (!p.plan.grouped) {          // one deterministic launch per member; stream order lets them share the scratch
    for (int i = 0; i < n; i++) {
      const int rc = mca_gemm_tn_acc_det(d[i].A, d[i].lda, d[i].B, d[i].ldb, d[i].C, d[i].ldc, R, d[i].N, d[i].K, scratch, scratch_floats, stream);
      if (rc != MCA_OK) return rc;
    }
    return MCA_OK;
  }
  const bool det = p.slots > 1;          // one split: the plain kernel over the same partition, one contributor per element
  tn_group g;
  int tiles = 0;
  int64_t off = 0;
  for (int i = 0; i < n; i++) {
    g.A[i] = d[i].A; g.B[i] = d[i].B;
    g.C[i] = det ? scratch + off : d[i].C;
    g.lda[i] = d[i].lda; g.ldb[i] = d[i].ldb; g.ldc[i] = det ? d[i].K : d[i].ldc;
    g.N[i] = (int)d[i].N; g.K[i] = (int)d[i].K;
    g.tiles_k[i] = (int)((d[i].K + 255) / 256);
    g.first_tile[i] = tiles;
    tiles += mca_tn_group_member_tiles(d[i].N, d[i].K);
    off += d[i].N * d[i].K;
  }
  for (int i = n; i <= MCA_TN_MAX_GROUP; i++) g.first_tile[i] = tiles;
  g.n = n; g.R = p.plan.part.R; g.tiles = p.plan.part.tiles;
  g.unit = p.plan.part.unit; g.n_full = p.plan.part.n_full; g.span = p.plan.part.span; g.own = p.plan.part.own;
  gemm_operands o = {};
  o.group = &g;
  int rc = det ? launch_det(p.plan.launch, o, stream) : launch(p.plan.launch, o, stream);
  if (rc != MCA_OK || !det) return rc;
  off = 0;
  for (int i = 0; i < n; i++) {
    rc = mca_det_reduce(scratch + off, p.slot_stride, p.slots, d[i].C, d[i].ldc, d[i].N, (int)d[i].K, stream);
    if (rc != MCA_OK) return rc;
    off += d[i].N * d[i].K;
  }
  return MCA_OK;
}

// ---- the plans themselves, for tests and tools (include/mca_hip_debug.h): the planners the entry points above call, with
// the current knob table; cus = 0 asks the runtime.  Nothing is launched and no device is touched.
extern "C" int mca_dbg_plan_gemm_nt(int entry, const mca_nt_problem* pr, int cus, mca_gemm_plan* out) {
  if (!pr || !out) return MCA_E_BADARG;
  if (cus <= 0) cus = num_cus();
  switch (entry) {
    case 0: *out = mca_plan_gemm_nt(*pr, mca_knobs, cus); return MCA_OK;
    case 1:
      if (!mca_nt_lnres_supported(pr->M, pr->N, pr->K)) return MCA_E_UNSUPPORTED;
      *out = mca_plan_gemm_nt_lnres(pr->M, pr->N); return MCA_OK;
    case 2: *out = mca_plan_gemm_nt_geglu_fwd(pr->M, pr->N, pr->K, mca_knobs, cus); return MCA_OK;
    case 3: *out = mca_plan_gemm_nt_geglu_bwd(pr->M, pr->N, pr->K, mca_knobs, cus); return MCA_OK;
    case 4: *out = mca_plan_gemm_nt_geglu_fwd_saved(pr->M, pr->N, pr->K, mca_knobs, cus); return MCA_OK;
    case 5: *out = mca_plan_gemm_nt_geglu_bwd_saved(pr->M, pr->N, pr->K, mca_knobs, cus); return MCA_OK;
    case 6:
      if (pr->M <= 0 || pr->N <= 0 || pr->K <= 0) return MCA_E_BADARG;
      if (mca_nt_rows_refusal(pr->M, pr->N, pr->K)) return mca_nt_rows_refusal(pr->M, pr->N, pr->K);
      *out = mca_plan_gemm_nt_res_lnbwd(pr->M); return MCA_OK;
    case 7:
      if (pr->M <= 0 || pr->N <= 0 || pr->K <= 0) return MCA_E_BADARG;
      if (mca_nt_rows_refusal(pr->M, pr->N, pr->K)) return mca_nt_rows_refusal(pr->M, pr->N, pr->K);
      *out = mca_plan_gemm_nt_res_lnbwd_tall(pr->M, mca_knobs, cus); return MCA_OK;
  }
  return MCA_E_BADARG;
}
extern "C" int mca_dbg_plan_gemm_nt_cb(int64_t M, int64_t N, int64_t K, uint64_t C, int64_t cbs, int cus, mca_gemm_plan* out) {
  if (!out || M <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  if (cus <= 0) cus = num_cus();
  return mca_plan_gemm_nt_cb(M, N, K, C, cbs, mca_knobs, cus, out) ? MCA_OK : MCA_E_UNSUPPORTED;
}
extern "C" const char* mca_dbg_gemm_kernel_name(int kernel) { return mca_gemm_kernel_name(kernel); }
extern "C" int mca_dbg_plan_gemm_tn(int64_t R, int64_t N, int64_t K, mca_gemm_plan* out) {
  if (!out || R <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  *out = mca_plan_gemm_tn(R, N, K, mca_knobs);
  return MCA_OK;
}
extern "C" int mca_dbg_plan_gemm_tn_group(const int64_t* N, const int64_t* K, int n, int64_t R, int cus, mca_tn_group_plan* out) {
  if (!N || !K || !out || n <= 0 || n > MCA_TN_MAX_GROUP || R <= 0) return MCA_E_BADARG;
  int tiles = 0;
  bool all_taken = true;
  for (int i = 0; i < n; i++) {
    const int t = mca_tn_group_member_tiles(N[i], K[i]);
    all_taken = all_taken && t > 0;
    tiles += t;
  }
  *out = mca_plan_gemm_tn_group(all_taken ? tiles : 0, n, R, mca_knobs, cus > 0 ? cus : num_cus());
  return MCA_OK;
}
extern "C" int mca_dbg_plan_gemm_tn_det(int64_t R, int64_t N, int64_t K, mca_tn_det_plan* out) {
  if (!out || R <= 0 || N <= 0 || K <= 0) return MCA_E_BADARG;
  *out = mca_plan_gemm_tn_det(R, N, K, mca_knobs);
  return MCA_OK;
}
extern "C" int mca_dbg_plan_gemm_tn_group_det(const int64_t* N, const int64_t* K, int n, int64_t R, int cus, mca_tn_group_det_plan* out) {
  if (!N || !K || !out || n <= 0 || n > MCA_TN_MAX_GROUP || R <= 0) return MCA_E_BADARG;
  *out = mca_plan_gemm_tn_group_det(N, K, n, R, mca_knobs, cus > 0 ? cus : num_cus());
  return MCA_OK;
}
