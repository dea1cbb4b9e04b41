// Downstream evaluation of the embeddings infer_accel_gpu.py writes: the retrieval rank metrics and the uniformity of the
// reference's lp_accel_gpu.py rank block (utils/metrics.py:20-27,72-98), and the per-step work of its linear / MLP probe
// (lp_accel_gpu.py:150-186).  fp32 throughout, no float atomics: every result is the same bits on every launch.
//
// One tile core serves the matrix products here: a 64x64 block of C[m, n] = sum_k A'[m, k] * B'[n, k] (or sum_k (A' - B')^2),
// 256 threads holding 4x4 outputs each, the K dimension staged through LDS 16 at a time.  Each output is ONE fmaf chain in
// ascending k from +0, so a value computed elsewhere with the same chain (the true target's cosine of the rank kernel) is
// bitwise the tile's value.  The chain runs on the vector ALUs; the fp32-input MFMA form (the same chain at about twice the
// rate) is the next step for the rank and pair kernels.  The row kernels (normalisation, probe head) are not tile-core
// products: they add lane-strided partials in a fixed xor tree, deterministic but not one k-ordered chain.
#include "common.h"

namespace {

constexpr int TILE = 64, KC = 16, LDSW = TILE + 4;

// NT: A' rows are A[(aidx ? aidx[m] : m) * lda + k], B' rows B[n * ldb + k] (row-major operands, reduction along the row).
// TN: A'[m, k] = A[k * lda + m], B'[n, k] = B[(bidx ? bidx[k] : k) * ldb + n], and B' column ones_col reads 1 (a bias
// gradient as one more output column).  SQDIFF: (a - b)^2 instead of a * b.
template <bool TN, bool SQDIFF>
__device__ __forceinline__ void tile_core(float (&acc)[4][4], const float* __restrict__ A, int64_t lda, const int32_t* __restrict__ aidx,
                                          int64_t M, int64_t m0, const float* __restrict__ B, int64_t ldb, const int32_t* __restrict__ bidx,
                                          int64_t N, int64_t n0, int64_t k0, int64_t k1, int64_t ones_col,
                                          float (*As)[LDSW], float (*Bs)[LDSW]) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int64_t kb = k0; kb < k1; kb += KC) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int e = tid + 256 * i;
      const int r = TN ? (e & 63) : (e >> 4), k = TN ? (e >> 6) : (e & 15);
      const int64_t kk = kb + k, m = m0 + r, n = n0 + r;
      float a = 0.f, b = 0.f;
      if (kk < k1) {
        if (!TN) {
          if (m < M) a = A[(int64_t)(aidx ? aidx[m] : m) * lda + kk];
          if (n < N) b = B[n * ldb + kk];
        } else {
          if (m < M) a = A[kk * lda + m];
          if (n < N) b = n == ones_col ? 1.f : B[(int64_t)(bidx ? bidx[kk] : kk) * ldb + n];
        }
      }
      As[k][r] = a;
      Bs[k][r] = b;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KC; k++) {
      const float4 a4 = *reinterpret_cast<const float4*>(&As[k][ty * 4]);
      const float4 b4 = *reinterpret_cast<const float4*>(&Bs[k][tx * 4]);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (SQDIFF) {
            const float d = av[i] - bv[j];
            acc[i][j] = fmaf(d, d, acc[i][j]);
          } else {
            acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
          }
        }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void zero_acc(float (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
}

// ---- y = x / max(||x||_2, 1e-8): one wave per row
__global__ __launch_bounds__(256) void rows_normalize_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                             int64_t n, int64_t d) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* xr = x + row * ldx;
  float s = 0.f;
  for (int64_t k = lane; k < d; k += 64) s = fmaf(xr[k], xr[k], s);
  s = wave_sum(s);
  const float nrm = fmaxf(sqrtf(s), 1e-8f);
  for (int64_t k = lane; k < d; k += 64) y[row * ldy + k] = xr[k] / nrm;
}

// ---- rank: s_true[r] by the tile's chain; rank[r] = 0
__global__ __launch_bounds__(256) void rank_true_kernel(const float* __restrict__ q, int64_t ldq, const int32_t* __restrict__ qidx, int64_t nq,
                                                        const float* __restrict__ t, int64_t ldt, int64_t d, float* __restrict__ s_true,
                                                        int32_t* __restrict__ rank) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nq) return;
  const int64_t i = qidx ? qidx[r] : r;
  const float* a = q + i * ldq;
  const float* b = t + i * ldt;
  float acc = 0.f;
  for (int64_t k = 0; k < d; k++) acc = fmaf(a[k], b[k], acc);
  s_true[r] = acc;
  rank[r] = 0;
}

// grid (query tiles, target chunks): each block counts s > s_true over the chunk's target tiles; LDS and global counters
// are integers (order-free)
__global__ __launch_bounds__(256) void rank_count_kernel(const float* __restrict__ q, int64_t ldq, const int32_t* __restrict__ qidx, int64_t nq,
                                                         const float* __restrict__ t, int64_t ldt, int64_t nt, int64_t d, int tiles_per_chunk,
                                                         const float* __restrict__ s_true, int32_t* __restrict__ rank) {
  __shared__ float As[KC][LDSW], Bs[KC][LDSW];
  __shared__ int cnt_s[TILE];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * TILE;
  float st[4];
  int cnt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; i++) st[i] = m0 + ty * 4 + i < nq ? s_true[m0 + ty * 4 + i] : 0.f;
  if (tid < TILE) cnt_s[tid] = 0;
  for (int tt = 0; tt < tiles_per_chunk; tt++) {
    const int64_t n0 = ((int64_t)blockIdx.y * tiles_per_chunk + tt) * TILE;
    if (n0 >= nt) break;
    float acc[4][4];
    zero_acc(acc);
    tile_core<false, false>(acc, q, ldq, qidx, nq, m0, t, ldt, nullptr, nt, n0, 0, d, -1, As, Bs);
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 4; j++) cnt[i] += (n0 + tx * 4 + j < nt && acc[i][j] > st[i]) ? 1 : 0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (cnt[i]) atomicAdd(&cnt_s[ty * 4 + i], cnt[i]);
  __syncthreads();
  if (tid < TILE && m0 + tid < nq && cnt_s[tid]) atomicAdd(&rank[m0 + tid], cnt_s[tid]);
}

// ---- top-k: the k best (score, index) pairs per query under ONE total order, so no result depends on the order of arrival
// a comes before b: the higher score, or on equal scores (+0 == -0) the lower index.  NaN never enters (filtered before).
__device__ __forceinline__ bool topk_before(float sa, int ia, float sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// grid (query tiles, target chunks), the rank kernel's shape.  LDS: per query row the chunk's best k pairs so far, sorted
// (dynamic: 64 * k * 8 bytes), and the survivors of the current tile as a 64 x 64 score image plus a 64-bit column mask per row
// (set with integer atomicOr).  After each tile a thread offers those of its 4 x 4 outputs that are candidates and come before
// the row's k-th entry; then each wave merges, row by row, the survivors into its 16 rows' lists: every element's place in the
// merged list is the number of elements before it, counted with wave broadcasts of a loop bounded by k + 64.  Every barrier is
// reached by the whole workgroup: the tile count is fixed at entry, the merge loops are per wave and hold no barrier.
// The chunk's lists go to ws_s / ws_i [chunk][query][k], padded with -inf / -1.
__global__ __launch_bounds__(256) void topk_chunk_kernel(const float* __restrict__ q, int64_t ldq, const int32_t* __restrict__ qidx, int64_t nq,
                                                         const float* __restrict__ t, int64_t ldt, int64_t nt, int64_t d,
                                                         const uint8_t* __restrict__ tvalid, const int32_t* __restrict__ exclude, int k,
                                                         int tiles_per_chunk, float* __restrict__ ws_s, int32_t* __restrict__ ws_i) {
  __shared__ float As[KC][LDSW], Bs[KC][LDSW];
  __shared__ float cand[TILE][TILE];
  __shared__ unsigned int cmask[TILE][2];
  __shared__ int cnt_s[TILE];
  extern __shared__ float best_dyn[];
  float* best_s = best_dyn;
  int* best_i = reinterpret_cast<int*>(best_dyn + TILE * k);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wv = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * TILE;
  const int64_t ntiles = (nt + TILE - 1) / TILE, tile0 = (int64_t)blockIdx.y * tiles_per_chunk;
  const int tiles = (int)(ntiles - tile0 < tiles_per_chunk ? ntiles - tile0 : tiles_per_chunk);
  int ex[4];
#pragma unroll
  for (int i = 0; i < 4; i++) ex[i] = (exclude && m0 + ty * 4 + i < nq) ? exclude[m0 + ty * 4 + i] : -1;
  if (tid < TILE) {
    cnt_s[tid] = 0;
    cmask[tid][0] = 0u;
    cmask[tid][1] = 0u;
  }
  for (int tt = 0; tt < tiles; tt++) {
    const int64_t n0 = (tile0 + tt) * TILE;
    float acc[4][4];
    zero_acc(acc);
    tile_core<false, false>(acc, q, ldq, qidx, nq, m0, t, ldt, nullptr, nt, n0, 0, d, -1, As, Bs);          // d >= 1: ends with a barrier
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t n = n0 + tx * 4 + j;
      ok[j] = n < nt && (!tvalid || tvalid[n] != 0);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = ty * 4 + i;
      if (m0 + r >= nq) continue;
      const bool full = cnt_s[r] == k;
      const float ks = full ? best_s[r * k + k - 1] : 0.f;
      const int ki = full ? best_i[r * k + k - 1] : 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int c = tx * 4 + j, n = (int)n0 + c;
        const float s = acc[i][j];
        if (ok[j] && n != ex[i] && s == s && (!full || topk_before(s, n, ks, ki))) {
          cand[r][c] = s;
          atomicOr(&cmask[r][c >> 5], 1u << (c & 31));
        }
      }
    }
    __syncthreads();
    for (int rr = 0; rr < TILE / 4; rr++) {
      const int r = wv * (TILE / 4) + rr;
      const uint32_t mlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmask[r][0]), mhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmask[r][1]);
      const uint64_t m = ((uint64_t)mhi << 32) | (uint64_t)mlo;
      if (m == 0) continue;
      const int n = __builtin_amdgcn_readfirstlane(cnt_s[r]);
      const bool has_l = lane < n, has_c = (m >> lane) & 1;
      const float ls = has_l ? best_s[r * k + lane] : 0.f, cs = has_c ? cand[r][lane] : 0.f;
      const int li = has_l ? best_i[r * k + lane] : 0, ci = (int)n0 + lane;
      int pos_l = lane, pos_c = 0;
      for (uint64_t mm = m; mm; mm &= mm - 1) {          // at most 64 survivors
        const int b = __builtin_ctzll(mm);
        const float xs = __shfl(cs, b, WAVE);
        const int xi = (int)n0 + b;
        pos_l += topk_before(xs, xi, ls, li) ? 1 : 0;
        pos_c += (b != lane && topk_before(xs, xi, cs, ci)) ? 1 : 0;
      }
      for (int e = 0; e < n; e++) {                      // n <= k
        const float ys = __shfl(ls, e, WAVE);
        const int yi = __shfl(li, e, WAVE);
        pos_c += topk_before(ys, yi, cs, ci) ? 1 : 0;
      }
      // every lane has read its own entry above; a wave's LDS accesses complete in program order
      if (has_l && pos_l < k) {
        best_s[r * k + pos_l] = ls;
        best_i[r * k + pos_l] = li;
      }
      if (has_c && pos_c < k) {
        best_s[r * k + pos_c] = cs;
        best_i[r * k + pos_c] = ci;
      }
      if (lane == 0) {
        const int total = n + __builtin_popcountll(m);
        cnt_s[r] = total < k ? total : k;
        cmask[r][0] = 0u;
        cmask[r][1] = 0u;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < TILE * k; e += 256) {
    const int r = e / k, c = e - r * k;
    if (m0 + r >= nq) break;
    const int64_t off = ((int64_t)blockIdx.y * nq + m0 + r) * k + c;
    const bool have = c < cnt_s[r];
    ws_s[off] = have ? best_s[e] : -__builtin_inff();
    ws_i[off] = have ? best_i[e] : -1;
  }
}

// one wave per query: the chunks' lists, each sorted and padded, merged one after the other into the wave's running list by
// the same counting (lane l holds entry l); a 64-entry LDS row per wave moves the entries to their places.  No block barrier.
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_i, int chunks, int64_t nq,
                                                         int k, float* __restrict__ score, int64_t lds, int32_t* __restrict__ index, int64_t ldi) {
  __shared__ float sm_s[4][TILE];
  __shared__ int sm_i[4][TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= nq) return;
  float ls = -__builtin_inff();
  int li = -1, n = 0;
  for (int c = 0; c < chunks; c++) {
    const int64_t off = ((int64_t)c * nq + r) * k;
    const float cs = lane < k ? ws_s[off + lane] : -__builtin_inff();
    const int ci = lane < k ? ws_i[off + lane] : -1;
    const int cn = __builtin_popcountll(__ballot(ci >= 0));          // the entries are a prefix of the k slots
    if (cn == 0) continue;
    int pos_l = lane, pos_c = lane;
    for (int e = 0; e < cn; e++) pos_l += topk_before(__shfl(cs, e, WAVE), __shfl(ci, e, WAVE), ls, li) ? 1 : 0;
    for (int e = 0; e < n; e++) pos_c += topk_before(__shfl(ls, e, WAVE), __shfl(li, e, WAVE), cs, ci) ? 1 : 0;
    if (lane < n && pos_l < k) {
      sm_s[wv][pos_l] = ls;
      sm_i[wv][pos_l] = li;
    }
    if (lane < cn && pos_c < k) {
      sm_s[wv][pos_c] = cs;
      sm_i[wv][pos_c] = ci;
    }
    n = n + cn < k ? n + cn : k;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    ls = lane < n ? sm_s[wv][lane] : -__builtin_inff();
    li = lane < n ? sm_i[wv][lane] : -1;
    __builtin_amdgcn_wave_barrier();          // the next chunk's stores stay behind these loads
  }
  if (lane < k) {
    score[r * lds + lane] = ls;
    index[r * ldi + lane] = li;
  }
}

// ---- sum_{i<j} exp(-t * d2_ij): grid (T, T) tiles, blocks below the diagonal write 0; fp64 per-tile partials
__global__ __launch_bounds__(256) void pair_gauss_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int64_t d, float t,
                                                         double* __restrict__ partials) {
  __shared__ float As[KC][LDSW], Bs[KC][LDSW];
  __shared__ double red[256];
  const int bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t slot = (int64_t)bi * gridDim.x + bj;
  if (bj < bi) {
    if (tid == 0) partials[slot] = 0.0;
    return;
  }
  const int64_t m0 = (int64_t)bi * TILE, n0 = (int64_t)bj * TILE;
  float acc[4][4];
  zero_acc(acc);
  tile_core<false, true>(acc, x, ldx, nullptr, n, m0, x, ldx, nullptr, n, n0, 0, d, -1, As, Bs);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t gi = m0 + ty * 4 + i, gj = n0 + tx * 4 + j;
      if (gi < gj && gj < n) s += (double)expf(-t * acc[i][j]);
    }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) partials[slot] = red[0];
}

__global__ __launch_bounds__(256) void pair_gauss_final_kernel(const double* __restrict__ partials, int64_t np, int64_t n,
                                                               double* __restrict__ sum_out, float* __restrict__ value_out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t i = tid; i < np; i += 256) s += partials[i];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double pairs = 0.5 * (double)n * (double)(n - 1);
    if (sum_out) sum_out[0] = red[0];
    if (value_out) value_out[0] = pairs > 0 ? (float)log(red[0] / pairs) : __builtin_nanf("");
  }
}

// ---- probe: counter-based dropout mask (hash_uniform24 of common.h over (seed, step, row in batch, unit))
__device__ __forceinline__ bool dropout_keep(uint64_t seed, int64_t step, int64_t row, int64_t unit, float p) {
  return hash_uniform24(seed, step, row, unit) >= p;
}

// Y[m, n] = act(X[idx[m]] . W[n] + bias[n]); act: 0 none, 1 ReLU, 2 dropout then ReLU (nn.Sequential order of the MLP probe)
__global__ __launch_bounds__(256) void probe_nt_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ xidx,
                                                       const float* __restrict__ w, int64_t ldw, const float* __restrict__ bias,
                                                       float* __restrict__ y, int64_t ldy, int64_t M, int64_t N, int64_t K, int act,
                                                       float p, uint64_t seed, int64_t step) {
  __shared__ float As[KC][LDSW], Bs[KC][LDSW];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * TILE, n0 = (int64_t)blockIdx.y * TILE;
  float acc[4][4];
  zero_acc(acc);
  tile_core<false, false>(acc, x, ldx, xidx, M, m0, w, ldw, nullptr, N, n0, 0, K, -1, As, Bs);
  const float scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
      if (m >= M || n >= N) continue;
      float z = acc[i][j] + (bias ? bias[n] : 0.f);
      if (act == 2) z = dropout_keep(seed, step, m, n, p) ? z * scale : 0.f;
      if (act >= 1) z = fmaxf(z, 0.f);
      y[m * ldy + n] = z;
    }
}

// one wave per batch row: logits z[l] = A[row] . W[l] + b[l] (lane-strided partials, fixed xor tree), loss, dz = dloss/dz /
// count, preds; dA[row, k] = sum_l dz[l] W[l, k], zeroed where A <= 0 and scaled by dact_scale (the ReLU + dropout backward
// of the MLP's hidden layer, read off its stored output); loss_part[block] = sum of the block's element losses
__global__ __launch_bounds__(256) void probe_head_kernel(const float* __restrict__ a, int64_t lda, const int32_t* __restrict__ aidx, int K,
                                                         const float* __restrict__ w, const float* __restrict__ bias, int L,
                                                         const float* __restrict__ labels, const int32_t* __restrict__ yidx, int64_t B,
                                                         int loss_type, float inv_count, float* __restrict__ pred, float* __restrict__ dz,
                                                         float* __restrict__ da, float dact_scale, float* __restrict__ loss_part) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  float loss_e = 0.f;
  if (row < B) {
    const int64_t src = aidx ? aidx[row] : row;
    float av[16];
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = (j * 64 + lane < K) ? a[src * lda + j * 64 + lane] : 0.f;
    float my_z = 0.f;
    for (int l = 0; l < L; l++) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (j * 64 + lane < K) s = fmaf(av[j], w[(int64_t)l * K + j * 64 + lane], s);
      s = wave_sum(s) + bias[l];
      if (lane == l) my_z = s;
    }
    float g = 0.f;
    if (lane < L) {
      const float yv = labels[(int64_t)(yidx ? yidx[row] : row) * L + lane], z = my_z, e = z - yv;
      if (loss_type == 0) {          // L1
        loss_e = fabsf(e);
        g = (float)((e > 0.f) - (e < 0.f));
      } else if (loss_type == 1) {   // MSE
        loss_e = e * e;
        g = 2.f * e;
      } else {                       // BCE with logits
        loss_e = fmaxf(z, 0.f) - z * yv + log1pf(expf(-fabsf(z)));
        g = 1.f / (1.f + expf(-z)) - yv;
      }
      g *= inv_count;
      pred[row * L + lane] = z;
      if (dz) dz[row * L + lane] = g;
    }
    if (da) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int k = j * 64 + lane;
        float s = 0.f;
        for (int l = 0; l < L; l++) {
          const float gl = __shfl(g, l, WAVE);
          if (k < K) s = fmaf(gl, w[(int64_t)l * K + k], s);
        }
        if (k < K) da[row * K + k] = av[j] > 0.f ? s * dact_scale : 0.f;
      }
    }
  }
  loss_e = wave_sum(loss_e);
  if (lane == 0) red[wv] = loss_e;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// partials[c][m][n] = sum over the rows of chunk c of A[r, m] * B[idx[r], n] (B column K reads 1: the bias gradient)
__global__ __launch_bounds__(256) void probe_tn_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb,
                                                       const int32_t* __restrict__ bidx, int64_t R, int64_t N, int64_t K, int64_t rows_per_chunk,
                                                       float* __restrict__ partials) {
  __shared__ float As[KC][LDSW], Bs[KC][LDSW];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t Kc = K + 1, m0 = (int64_t)blockIdx.x * TILE, n0 = (int64_t)blockIdx.y * TILE;
  const int64_t r0 = (int64_t)blockIdx.z * rows_per_chunk, r1 = r0 + rows_per_chunk < R ? r0 + rows_per_chunk : R;
  float acc[4][4];
  zero_acc(acc);
  tile_core<true, false>(acc, a, lda, nullptr, N, m0, b, ldb, bidx, Kc, n0, r0, r1, K, As, Bs);
  float* out = partials + (int64_t)blockIdx.z * N * Kc;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t m = m0 + ty * 4 + i, n = n0 + tx * 4 + j;
      if (m < N && n < Kc) out[m * Kc + n] = acc[i][j];
    }
}

// gw[m, n] (n < K) and gb[m] (n == K) = sum over chunks c = 0, 1, ... of partials[c][m][n]
__global__ __launch_bounds__(256) void probe_reduce_kernel(const float* __restrict__ partials, int chunks, int64_t N, int64_t K,
                                                           float* __restrict__ gw, float* __restrict__ gb) {
  const int64_t Kc = K + 1, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * Kc) return;
  float s = 0.f;
  for (int c = 0; c < chunks; c++) s += partials[(int64_t)c * N * Kc + e];
  const int64_t m = e / Kc, n = e % Kc;
  if (n < K) gw[m * K + n] = s;
  else gb[m] = s;
}

// acc[0] += (sum of the block partials, lane-strided then a fixed xor tree) / count
__global__ __launch_bounds__(64) void probe_loss_accum_kernel(const float* __restrict__ part, int64_t n, float count, float* __restrict__ acc) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 64) s += part[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) acc[0] += s / count;
}

constexpr int RANK_TILES_PER_CHUNK = 16;
constexpr int TOPK_TILES_PER_CHUNK = 16;          // 1024 targets per workgroup: the rank kernel's grid
constexpr int64_t PROBE_ROWS_PER_CHUNK = 128;

}  // namespace

extern "C" int mca_rows_normalize_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t n, int64_t d, mca_stream_t stream) {
  if (!x || !y || n < 0 || d <= 0 || ldx < d || ldy < d) return MCA_E_BADARG;
  if (n == 0) return MCA_OK;
  hipLaunchKernelGGL(rows_normalize_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), x, ldx, y, ldy, n, d);
  return launch_status();
}

extern "C" int mca_cosine_rank_f32(const float* q, int64_t ldq, const int32_t* qidx, int64_t nq, const float* t, int64_t ldt, int64_t nt,
                                   int64_t d, float* s_true, int32_t* rank, mca_stream_t stream) {
  if (!q || !t || !s_true || !rank || nq < 0 || nt <= 0 || d <= 0 || ldq < d || ldt < d) return MCA_E_BADARG;
  if (!qidx && nq > nt) return MCA_E_BADARG;          // query r's true target is target r
  if (nq == 0) return MCA_OK;
  hipLaunchKernelGGL(rank_true_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, as_stream(stream), q, ldq, qidx, nq, t, ldt, d,
                     s_true, rank);
  const int64_t ntiles = (nt + TILE - 1) / TILE, chunks = (ntiles + RANK_TILES_PER_CHUNK - 1) / RANK_TILES_PER_CHUNK;
  hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)((nq + TILE - 1) / TILE), (unsigned)chunks), dim3(256), 0, as_stream(stream), q, ldq,
                     qidx, nq, t, ldt, nt, d, RANK_TILES_PER_CHUNK, s_true, rank);
  return launch_status();
}

static int64_t topk_chunks(int64_t nt) {
  const int64_t ntiles = (nt + TILE - 1) / TILE;
  return (ntiles + TOPK_TILES_PER_CHUNK - 1) / TOPK_TILES_PER_CHUNK;
}

extern "C" int64_t mca_cosine_topk_workspace(int64_t nq, int64_t nt, int k) {
  if (nq < 0 || nt < 0 || k < 1 || k > MCA_TOPK_MAX) return -1;
  return topk_chunks(nt) * nq * k * (int64_t)(sizeof(float) + sizeof(int32_t));
}

extern "C" int mca_cosine_topk_f32(const float* q, int64_t ldq, const int32_t* qidx, int64_t nq, const float* t, int64_t ldt, int64_t nt,
                                   int64_t d, const uint8_t* tvalid, const int32_t* exclude, int k, void* ws, int64_t ws_bytes, float* score,
                                   int64_t lds, int32_t* index, int64_t ldi, mca_stream_t stream) {
  if (!q || !score || !index || (nt > 0 && !t) || nq < 0 || nt < 0 || d < 1 || k < 1) return MCA_E_BADARG;
  if (k > MCA_TOPK_MAX) return MCA_E_UNSUPPORTED;
  if (ldq < d || ldt < d || lds < k || ldi < k) return MCA_E_BADARG;
  const int64_t need = mca_cosine_topk_workspace(nq, nt, k), chunks = topk_chunks(nt);
  if (ws_bytes < need || (need > 0 && !ws)) return MCA_E_BADARG;
  if (reinterpret_cast<uintptr_t>(ws) % alignof(float)) return MCA_E_ALIGN;
  if (nt > INT32_MAX || chunks > 65535) return MCA_E_UNSUPPORTED;          // indices are int32; chunks are grid.y
  if (nq == 0) return MCA_OK;
  float* ws_s = static_cast<float*>(ws);
  int32_t* ws_i = reinterpret_cast<int32_t*>(ws_s + chunks * nq * k);
  if (chunks > 0)
    hipLaunchKernelGGL(topk_chunk_kernel, dim3((unsigned)((nq + TILE - 1) / TILE), (unsigned)chunks), dim3(256),
                       (size_t)TILE * k * (sizeof(float) + sizeof(int32_t)), as_stream(stream), q, ldq, qidx, nq, t, ldt, nt, d, tvalid, exclude,
                       k, TOPK_TILES_PER_CHUNK, ws_s, ws_i);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, as_stream(stream), ws_s, ws_i, (int)chunks, nq, k, score,
                     lds, index, ldi);
  return launch_status();
}

extern "C" int64_t mca_pair_gauss_workspace(int64_t n) {
  const int64_t tiles = n > 0 ? (n + TILE - 1) / TILE : 1;
  return tiles * tiles;
}

extern "C" int mca_pair_gauss_sum_f32(const float* x, int64_t ldx, int64_t n, int64_t d, float t, double* partials, int64_t n_partials,
                                      double* sum_out, float* value_out, mca_stream_t stream) {
  if (!partials || n < 0 || d <= 0 || (n > 0 && (!x || ldx < d)) || n_partials < mca_pair_gauss_workspace(n)) return MCA_E_BADARG;
  if (n > (int64_t)TILE * 65535) return MCA_E_UNSUPPORTED;
  int64_t np = 0;
  if (n > 1) {
    const int64_t tiles = (n + TILE - 1) / TILE;
    np = tiles * tiles;
    hipLaunchKernelGGL(pair_gauss_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(256), 0, as_stream(stream), x, ldx, n, d, t, partials);
  }
  hipLaunchKernelGGL(pair_gauss_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), partials, np, n, sum_out, value_out);
  return launch_status();
}

extern "C" int mca_probe_nt_f32(const float* x, int64_t ldx, const int32_t* xidx, const float* w, int64_t ldw, const float* bias, float* y,
                                int64_t ldy, int64_t M, int64_t N, int64_t K, int act, float p, uint64_t seed, int64_t step,
                                mca_stream_t stream) {
  if (!x || !w || !y || M <= 0 || N <= 0 || K <= 0 || ldx < K || ldw < K || ldy < N || act < 0 || act > 2) return MCA_E_BADARG;
  if (M > (int64_t)TILE * 65535 || N > (int64_t)TILE * 65535) return MCA_E_UNSUPPORTED;
  hipLaunchKernelGGL(probe_nt_kernel, dim3((unsigned)((M + TILE - 1) / TILE), (unsigned)((N + TILE - 1) / TILE)), dim3(256), 0,
                     as_stream(stream), x, ldx, xidx, w, ldw, bias, y, ldy, M, N, K, act, p, seed, step);
  return launch_status();
}

extern "C" int64_t mca_probe_head_blocks(int64_t B) { return (B + 3) / 4; }

extern "C" int mca_probe_head_f32(const float* a, int64_t lda, const int32_t* aidx, int64_t K, const float* w, const float* bias, int64_t L,
                                  const float* labels, const int32_t* yidx, int64_t B, int loss_type, float* pred, float* dz, float* da,
                                  float dact_scale, float* loss_part, mca_stream_t stream) {
  if (!a || !w || !bias || !labels || !pred || !loss_part || B <= 0 || K <= 0 || L <= 0 || lda < K || loss_type < 0 || loss_type > 2)
    return MCA_E_BADARG;
  if (K > 1024 || L > 64) return MCA_E_UNSUPPORTED;
  hipLaunchKernelGGL(probe_head_kernel, dim3((unsigned)mca_probe_head_blocks(B)), dim3(256), 0, as_stream(stream), a, lda, aidx, (int)K, w,
                     bias, (int)L, labels, yidx, B, loss_type, 1.f / (float)(B * L), pred, dz, da, dact_scale, loss_part);
  return launch_status();
}

extern "C" int64_t mca_probe_tn_workspace(int64_t R, int64_t N, int64_t K) {
  return ((R + PROBE_ROWS_PER_CHUNK - 1) / PROBE_ROWS_PER_CHUNK) * N * (K + 1);
}

extern "C" int mca_probe_tn_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const int32_t* bidx, int64_t R, int64_t N, int64_t K,
                                float* partials, int64_t n_partials, float* gw, float* gb, mca_stream_t stream) {
  if (!a || !b || !partials || !gw || !gb || R <= 0 || N <= 0 || K <= 0 || lda < N || ldb < K) return MCA_E_BADARG;
  if (n_partials < mca_probe_tn_workspace(R, N, K)) return MCA_E_BADARG;
  const int64_t chunks = (R + PROBE_ROWS_PER_CHUNK - 1) / PROBE_ROWS_PER_CHUNK;
  if (chunks > 65535 || (N + TILE - 1) / TILE > 65535) return MCA_E_UNSUPPORTED;
  hipLaunchKernelGGL(probe_tn_kernel, dim3((unsigned)((N + TILE - 1) / TILE), (unsigned)((K + 1 + TILE - 1) / TILE), (unsigned)chunks), dim3(256),
                     0, as_stream(stream), a, lda, b, ldb, bidx, R, N, K, PROBE_ROWS_PER_CHUNK, partials);
  hipLaunchKernelGGL(probe_reduce_kernel, dim3((unsigned)((N * (K + 1) + 255) / 256)), dim3(256), 0, as_stream(stream), partials, (int)chunks,
                     N, K, gw, gb);
  return launch_status();
}

extern "C" int mca_probe_loss_accum(const float* loss_part, int64_t n, int64_t count, float* acc, mca_stream_t stream) {
  if (!loss_part || !acc || n <= 0 || count <= 0) return MCA_E_BADARG;
  hipLaunchKernelGGL(probe_loss_accum_kernel, dim3(1), dim3(64), 0, as_stream(stream), loss_part, n, (float)count, acc);
  return launch_status();
}
