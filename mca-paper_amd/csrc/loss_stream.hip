// All-pairs contrastive loss with temperature, forward + backward, STREAMING form: the formulas of loss.hip's header comments with
// no (B, B) matrix in memory.  Reference lines replaced: those of loss.hip (model.py:175-233 and
// utils/contrastive_loss_with_temperature.py:40-108), for a gathered batch far beyond what one step's activations hold
// (mca-paper_amd/cached.py).
//
// A term t has the Gram matrix G = A Bᵀ (A = slot_a rows, B = slot_b rows of pooled_all) and logits l = T G.  Both directions of the
// term are the same computation on an OWNER side X and an OTHER side Y:
//     dir 0:  X = A, Y = B   (row statistics of l,    gradient of the slot_a rows)
//     dir 1:  X = B, Y = A   (column statistics of l, gradient of the slot_b rows)
// so S = X Yᵀ is l / T or its transpose, and dG as seen from the owner is
//     dG[x][y] = T ( w_x (exp(l - lse_own[x]) - [x == y]) + w_y (exp(l - lse_oth[y]) - [x == y]) ),      dX[x] = sum_y dG[x][y] Y[y].
//
// stream_stats_kernel   grid (ceil(B / TI), 2, T): a strip of TI owner rows against every TJ-row tile of the other side; Sᵀ tile on
//                       the fp32 MFMA (mfma(Y, X): a lane then holds 16 logits of ONE owner row), online softmax per lane, the 8
//                       lanes of a row combined in a fixed order.  Writes lse, E / S (the temperature derivative) and the diagonal.
// stream_reduce_kernel  one block: counts, per-term losses, w[t][r], the outputs of the local rank (loss.hip's reduce_terms_kernel
//                       with its LDS arrays in the workspace, so that every W = B / b_local is accepted).
// stream_grad_kernel    grid (ceil(b_local / TI), R): a strip of local rows of ONE slot; for every (term, dir) whose owner slot it
//                       is, in term order: recompute the Sᵀ tile, form dG in LDS, and add dG · Y into TI x D accumulators on the fp32
//                       MFMA.  One fma chain per output element, over (term, dir, y) in that order: no atomics, the same bytes every
//                       launch; a slot no term names is written as zeros.
// Arithmetic: v_mfma_f32_32x32x2_f32 only (exact fp32 products, fp32 accumulation, k ascending), zero fill past B and D.
#include "common.h"

#define ST_TI 32          // owner rows of a block
#define ST_TJ 128         // other-side rows of a tile step: 4 waves x 32
#define ST_TK 32          // columns of D staged per step
#define ST_DMAX 512       // the gradient accumulators hold TI x 512: 4 waves x 4 sub-tiles of 32 columns
#define ST_NEG (-3.0e38f)

namespace {

__device__ __forceinline__ bool st_term_valid(const mca_loss_term& tm, uint32_t present) {
  return ((present & tm.and_bits) == tm.and_bits) && (tm.or_bits == 0 || (present & tm.or_bits) != 0);
}

// row of a 32x32 MFMA result held in register r of a lane of half h (column = lane & 31)
__device__ __forceinline__ int st_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[r] = S[x = lane & 31][y = 32 wave + st_row(r, lane >> 5)] for the TI x TJ tile at (x0, j0): sum over d ascending.
// Xs / Ys: the staging buffers of the block.  Every thread of the block calls this (it synchronises).
__device__ __forceinline__ f32x16 st_gram_tile(const float* __restrict__ pooled, int R, int D, int slot_x, int slot_y, int x0, int x_end,
                                               int j0, int B, float (*Xs)[ST_TK + 1], float (*Ys)[ST_TK + 1]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  const int kc = tid & 31, rr = tid >> 5;          // a thread stages column kc of rows rr, rr + 8, ...
  float xr[ST_TI / 8], yr[ST_TJ / 8];              // the next chunk, loaded while the matrix cores work on this one
  auto fetch = [&](int k0) {
    const bool kin = k0 + kc < D;
#pragma unroll
    for (int p = 0; p < ST_TI / 8; p++) {
      const int x = x0 + rr + 8 * p;
      xr[p] = (kin && x < x_end) ? pooled[((int64_t)x * R + slot_x) * D + k0 + kc] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < ST_TJ / 8; p++) {
      const int y = j0 + rr + 8 * p;
      yr[p] = (kin && y < B) ? pooled[((int64_t)y * R + slot_y) * D + k0 + kc] : 0.f;
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += ST_TK) {
    __syncthreads();          // the reads of the chunk before are done
#pragma unroll
    for (int p = 0; p < ST_TI / 8; p++) Xs[rr + 8 * p][kc] = xr[p];
#pragma unroll
    for (int p = 0; p < ST_TJ / 8; p++) Ys[rr + 8 * p][kc] = yr[p];
    __syncthreads();
    if (k0 + ST_TK < D) fetch(k0 + ST_TK);
#pragma unroll
    for (int kk = 0; kk < ST_TK / 2; kk++)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ys[32 * wv + l31][2 * kk + h], Xs[l31][2 * kk + h], acc, 0, 0, 0);
  }
  return acc;
}

__global__ __launch_bounds__(256) void stream_stats_kernel(const float* __restrict__ pooled, const mca_loss_term* __restrict__ terms,
                                                            const float* __restrict__ logit_scale, float* __restrict__ lse,
                                                            float* __restrict__ erat, float* __restrict__ diag, int T, int B, int R, int D) {
  __shared__ float Xs[ST_TI][ST_TK + 1], Ys[ST_TJ][ST_TK + 1], part[8][ST_TI][3];
  const int t = blockIdx.z, dir = blockIdx.y, x0 = blockIdx.x * ST_TI;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int slot_x = dir ? terms[t].slot_b : terms[t].slot_a, slot_y = dir ? terms[t].slot_a : terms[t].slot_b;
  const float Tm = expf(*logit_scale);
  const int x = x0 + l31;
  float m = ST_NEG, s = 0.f, e = 0.f;
  for (int j0 = 0; j0 < B; j0 += ST_TJ) {
    const f32x16 acc = st_gram_tile(pooled, R, D, slot_x, slot_y, x0, B, j0, B, Xs, Ys);
    float l[16], mt = ST_NEG;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int y = j0 + 32 * wv + st_row(r, h);
      l[r] = Tm * acc[r];
      if (y < B) mt = fmaxf(mt, l[r]);
      if (dir == 0 && y == x && x < B) diag[(int64_t)t * B + x] = l[r];
    }
    const float mn = fmaxf(m, mt), sc = expf(m - mn);
    s *= sc; e *= sc;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int y = j0 + 32 * wv + st_row(r, h);
      if (y < B) {
        const float p = expf(l[r] - mn);
        s += p; e += p * l[r];
      }
    }
    m = mn;
  }
  __syncthreads();
  part[2 * wv + h][l31][0] = m; part[2 * wv + h][l31][1] = s; part[2 * wv + h][l31][2] = e;
  __syncthreads();
  if (tid < ST_TI && x0 + tid < B) {
    float M = part[0][tid][0];
    for (int k = 1; k < 8; k++) M = fmaxf(M, part[k][tid][0]);
    float S = 0.f, E = 0.f;
    for (int k = 0; k < 8; k++) {
      const float f = expf(part[k][tid][0] - M);
      S += part[k][tid][1] * f; E += part[k][tid][2] * f;
    }
    const int64_t o = ((int64_t)dir * T + t) * B + x0 + tid;
    lse[o] = M + logf(S);
    erat[o] = E / S;
  }
}

// n, s, ds, w: (T, W) each, in the workspace.  One block.
__global__ __launch_bounds__(256) void stream_reduce_kernel(const float* __restrict__ lse, const float* __restrict__ erat,
                                                             const float* __restrict__ diag, const uint32_t* __restrict__ present,
                                                             const mca_loss_term* __restrict__ terms, int T, int B, int b_local, int row0,
                                                             float* __restrict__ n, float* __restrict__ s, float* __restrict__ ds,
                                                             float* __restrict__ w, float* __restrict__ term_loss, float* __restrict__ loss,
                                                             float* __restrict__ d_logit_scale) {
  const int W = B / b_local;
  const int64_t TB = (int64_t)T * B;
  for (int idx = threadIdx.x; idx < T * W; idx += 256) {
    const int t = idx / W, r = idx % W;
    float cnt = 0.f, sum = 0.f, dsum = 0.f;
    for (int i = r * b_local; i < (r + 1) * b_local; i++) {
      if (st_term_valid(terms[t], present[i])) {
        const int64_t o = (int64_t)t * B + i;
        const float dg = diag[o];
        cnt += 1.f; sum += (lse[o] - dg) + (lse[TB + o] - dg); dsum += (erat[o] - dg) + (erat[TB + o] - dg);
      }
    }
    n[idx] = cnt; s[idx] = sum; ds[idx] = dsum;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < W; r += 256) {
    float nl = 0.f;
    for (int t = 0; t < T; t++) nl += n[t * W + r] > 0.f ? 1.f : 0.f;
    const float denom = nl > 0.f ? nl : 1.f;
    for (int t = 0; t < T; t++) w[t * W + r] = n[t * W + r] > 0.f ? 1.f / (2.f * n[t * W + r] * denom) : 0.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int r = row0 / b_local;
    float tot = 0.f, nl = 0.f, dtot = 0.f;
    for (int t = 0; t < T; t++) {
      const float cnt = n[t * W + r];
      if (cnt > 0.f) {
        const float l = s[t * W + r] / (2.f * cnt);
        term_loss[t] = l; tot += l; nl += 1.f; dtot += ds[t * W + r] / (2.f * cnt);
      } else term_loss[t] = __uint_as_float(0x7fc00000u);
    }
    const float denom = nl > 0.f ? nl : 1.f;
    *loss = tot / denom;
    *d_logit_scale = dtot / denom;
  }
}

__global__ __launch_bounds__(256) void stream_grad_kernel(const float* __restrict__ pooled, const uint32_t* __restrict__ present,
                                                           const mca_loss_term* __restrict__ terms, int T,
                                                           const float* __restrict__ logit_scale, const float* __restrict__ lse,
                                                           const float* __restrict__ w, int B, int b_local, int row0, int R, int D,
                                                           float* __restrict__ d_pooled) {
  __shared__ float Xs[ST_TI][ST_TK + 1], Ys[ST_TJ][ST_TK + 1], dGs[ST_TI][ST_TJ + 1], ylse[ST_TJ], yw[ST_TJ], xlse[ST_TI], xw[ST_TI];
  const int slot = blockIdx.y, x0 = row0 + blockIdx.x * ST_TI, x_end = row0 + b_local, W = B / b_local;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const float Tm = expf(*logit_scale);
  const int dbase = wv * (ST_DMAX / 4);
  f32x16 out[4];
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int r = 0; r < 16; r++) out[c][r] = 0.f;
  for (int t = 0; t < T; t++) {
    for (int dir = 0; dir < 2; dir++) {
      const int own = dir ? terms[t].slot_b : terms[t].slot_a, oth = dir ? terms[t].slot_a : terms[t].slot_b;
      if (own != slot) continue;          // (the same for every thread of the block)
      __syncthreads();
      if (tid < ST_TI) {
        const int x = x0 + tid;
        const bool in = x < x_end;
        xlse[tid] = in ? lse[((int64_t)dir * T + t) * B + x] : 0.f;
        xw[tid] = (in && st_term_valid(terms[t], present[x])) ? w[t * W + x / b_local] : 0.f;
      }
      for (int j0 = 0; j0 < B; j0 += ST_TJ) {
        if (tid < ST_TJ) {
          const int y = j0 + tid;
          const bool in = y < B;
          ylse[tid] = in ? lse[((int64_t)(1 - dir) * T + t) * B + y] : 0.f;
          yw[tid] = (in && st_term_valid(terms[t], present[y])) ? w[t * W + y / b_local] : 0.f;
        }
        const f32x16 acc = st_gram_tile(pooled, R, D, own, oth, x0, x_end, j0, B, Xs, Ys);
        const int x = x0 + l31;
        const float wx = xw[l31], lx = xlse[l31];
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int yl = 32 * wv + st_row(r, h), y = j0 + yl;
          const float l = Tm * acc[r], eq = x == y ? 1.f : 0.f, wy = yw[yl];
          float g = 0.f;
          if (wx != 0.f) g += wx * (expf(l - lx) - eq);
          if (wy != 0.f) g += wy * (expf(l - ylse[yl]) - eq);
          dGs[l31][yl] = (y < B && x < x_end) ? Tm * g : 0.f;
        }
        __syncthreads();
        // out[x][d] += sum over the tile's y of dG[x][y] Y[y][d]: A = dG (row x on the lane), B = Y rows straight from memory
#pragma unroll 4
        for (int sI = 0; sI < ST_TJ / 2; sI++) {
          const int y = j0 + 2 * sI + h;
          const float a = dGs[l31][2 * sI + h];
          const float* yrow = pooled + ((int64_t)(y < B ? y : 0) * R + oth) * D;
#pragma unroll
          for (int c = 0; c < 4; c++) {
            if (dbase + 32 * c < D) {          // (the same for every lane of the wave)
              const int d = dbase + 32 * c + l31;
              const float bv = (y < B && d < D) ? yrow[d] : 0.f;
              out[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, out[c], 0, 0, 0);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int d = dbase + 32 * c + l31;
    if (d < D) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int x = x0 + st_row(r, h);
        if (x < x_end) d_pooled[((int64_t)(x - row0) * R + slot) * D + d] = out[c][r];
      }
    }
  }
}

}  // namespace

// The tile constants and the workspace of one call, stated once: out = {TI, TJ, TK, DMAX, lse offset, lse bytes, erat offset, erat
// bytes, diag offset, diag bytes, n/s/ds offset, n/s/ds bytes, w offset, w bytes}.  lse and erat are (2, T, B) fp32 (direction 0:
// rows, 1: columns), diag (T, B), n/s/ds three (T, W) arrays and w (T, W), each with room for W = B.  Pure host code.
extern "C" int mca_dbg_contrastive_stream_layout(int B, int T, int64_t* out) {
  if (!out || B <= 0 || T <= 0) return MCA_E_BADARG;
  const int64_t tb = (int64_t)T * B * 4;
  out[0] = ST_TI; out[1] = ST_TJ; out[2] = ST_TK; out[3] = ST_DMAX;
  out[4] = 0; out[5] = 2 * tb;
  out[6] = 2 * tb; out[7] = 2 * tb;
  out[8] = 4 * tb; out[9] = tb;
  out[10] = 5 * tb; out[11] = 3 * tb;
  out[12] = 8 * tb; out[13] = tb;
  return MCA_OK;
}

extern "C" int64_t mca_contrastive_stream_workspace_bytes(int B, int T, int R, int D) {
  (void)R; (void)D;
  int64_t lay[14];
  if (mca_dbg_contrastive_stream_layout(B, T, lay) != MCA_OK) return 0;
  return lay[12] + lay[13] + 256;
}

extern "C" int mca_contrastive_stream_fwd_bwd(const float* pooled_all, const uint32_t* present_all, const mca_loss_term* terms,
                                              int T, const float* logit_scale, int B, int b_local, int row0, int R, int D,
                                              float* term_loss, float* loss, float* d_pooled, float* d_logit_scale,
                                              void* workspace, int64_t workspace_bytes, mca_stream_t stream) {
  if (!pooled_all || !present_all || !terms || !logit_scale || !term_loss || !loss || !d_pooled || !d_logit_scale || !workspace)
    return MCA_E_BADARG;
  if (T <= 0 || B <= 0 || b_local <= 0 || B % b_local || row0 % b_local || row0 < 0 || row0 + b_local > B || R <= 0 || D <= 0)
    return MCA_E_BADARG;
  if (workspace_bytes < mca_contrastive_stream_workspace_bytes(B, T, R, D)) return MCA_E_BADARG;
  if (D > ST_DMAX || T > 65535 || R > 65535) return MCA_E_UNSUPPORTED;
  int64_t lay[14];
  mca_dbg_contrastive_stream_layout(B, T, lay);
  char* base = reinterpret_cast<char*>(workspace);
  float* lse = reinterpret_cast<float*>(base + lay[4]);
  float* erat = reinterpret_cast<float*>(base + lay[6]);
  float* diag = reinterpret_cast<float*>(base + lay[8]);
  float* red = reinterpret_cast<float*>(base + lay[10]);
  float* w = reinterpret_cast<float*>(base + lay[12]);
  const int64_t TW = (int64_t)T * (B / b_local);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(stream_stats_kernel, dim3((B + ST_TI - 1) / ST_TI, 2, T), dim3(256), 0, s, pooled_all, terms, logit_scale, lse,
                     erat, diag, T, B, R, D);
  hipLaunchKernelGGL(stream_reduce_kernel, dim3(1), dim3(256), 0, s, lse, erat, diag, present_all, terms, T, B, b_local, row0, red,
                     red + TW, red + 2 * TW, w, term_loss, loss, d_logit_scale);
  hipLaunchKernelGGL(stream_grad_kernel, dim3((b_local + ST_TI - 1) / ST_TI, R), dim3(256), 0, s, pooled_all, present_all, terms, T,
                     logit_scale, lse, w, B, b_local, row0, R, D, d_pooled);
  return launch_status();
}
