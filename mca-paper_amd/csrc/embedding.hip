// Token tables (encoders.py:17-37 TokenEncoder = nn.Embedding(max_norm = 1), as SequenceEncoder :145-166 and SparseTabularEncoder
// :100-120 use it): rows gathered by index with the touched-rows-only in-place renormalisation, and the table gradient summed by
// index, with fp32 atomics or in a fixed order.  An index outside [0, vocab) is never turned into an address.
#include "common.h"

// the table row token i names, or -1 when its index is outside [0, vocab)
__device__ __forceinline__ int64_t token_row(const void* __restrict__ idx, int idx_bytes, int64_t i, int64_t vocab) {
  const int64_t v = idx_bytes == 8 ? reinterpret_cast<const int64_t*>(idx)[i] : (int64_t)reinterpret_cast<const int32_t*>(idx)[i];
  return (v >= 0 && v < vocab) ? v : -1;
}

// ---- forward, launch 1 of 3: marker[v] = 1 for every row some token names; *flag |= oob_bit for an index out of range
__global__ __launch_bounds__(256) void embedding_mark_kernel(const void* __restrict__ idx, int idx_bytes, int64_t rows, int64_t vocab,
                                                              int32_t* __restrict__ marker, int32_t* __restrict__ flag, int oob_bit) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256) {
    const int64_t v = token_row(idx, idx_bytes, i, vocab);
    if (v >= 0) marker[v] = 1;          // (every writer stores 1)
    else bad = true;
  }
  if (flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, oob_bit);
}

// ---- launch 2: every marked row with L2 norm > max_norm is rescaled in place by max_norm / (norm + 1e-7), once, by one
// wavefront (mca_embedding_renorm's arithmetic), and its marker goes back to 0.  A wavefront takes RENORM_CHUNK markers at a time
// and walks the set ones: a small chunk, so that a densely touched stretch of the table is spread over many wavefronts.
#define RENORM_CHUNK 16
__global__ __launch_bounds__(256) void embedding_renorm_marked_kernel(float* __restrict__ w, int64_t vocab, int cols, float max_norm,
                                                                       int32_t* __restrict__ marker) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t base = wave * RENORM_CHUNK; base < vocab; base += nwaves * RENORM_CHUNK) {
    const int64_t mine = base + lane;
    const bool marked = lane < RENORM_CHUNK && mine < vocab && marker[mine] != 0;
    unsigned long long todo = __ballot(marked);
    while (todo) {
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      float* wr = w + (base + k) * cols;
      float s = 0.f;
      for (int c = lane; c < cols; c += 64) s += wr[c] * wr[c];
      const float nrm = sqrtf(wave_sum(s));
      if (nrm > max_norm) {
        const float sc = max_norm / (nrm + 1e-7f);
        for (int c = lane; c < cols; c += 64) wr[c] *= sc;
      }
    }
    if (marked) marker[mine] = 0;
  }
}

// ---- launch 3: dst row i (=|+=) table[idx[i]] (+ add[i % period]); one wavefront per token, 16-byte pieces
__global__ __launch_bounds__(256) void embedding_gather_kernel(const float* __restrict__ table, int64_t vocab, int cols,
                                                                const void* __restrict__ idx, int idx_bytes, int64_t rows, int64_t period,
                                                                const float* __restrict__ add, float* __restrict__ dst, int64_t ldd,
                                                                int64_t dst_bstride, int accumulate) {
  const int lane = threadIdx.x & 63, c4n = cols / 4;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (int64_t)gridDim.x * 4) {
    const int64_t v = token_row(idx, idx_bytes, i, vocab);
    const int64_t prow = i % period;
    if (v < 0 && !add && accumulate) continue;          // nothing to add
    const float4* tr = v >= 0 ? reinterpret_cast<const float4*>(table + v * cols) : nullptr;
    const float4* ar = add ? reinterpret_cast<const float4*>(add + prow * cols) : nullptr;
    float4* dr = reinterpret_cast<float4*>(dst + (i / period) * dst_bstride + prow * ldd);
    for (int c = lane; c < c4n; c += 64) {
      float4 t = tr ? tr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (ar) { const float4 a = ar[c]; t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w; }
      if (accumulate) { const float4 o = dr[c]; t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w; }
      dr[c] = t;
    }
  }
}

static inline unsigned wave_grid(int64_t waves) {
  int64_t blocks = (waves + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int mca_embedding_lookup(float* table, int64_t vocab, int cols, float max_norm, const void* idx, int idx_bytes,
                                    int64_t rows, int64_t period, const float* add, float* dst, int64_t ldd, int64_t dst_bstride,
                                    int accumulate, int32_t* marker, int32_t* flag, int oob_bit, mca_stream_t stream) {
  if (!table || !idx || !dst || !marker || vocab <= 0 || cols <= 0 || rows < 0 || period <= 0) return MCA_E_BADARG;
  if ((idx_bytes != 4 && idx_bytes != 8) || (flag && oob_bit == 0)) return MCA_E_BADARG;
  if (cols % 4 || ldd % 4 || dst_bstride % 4 || (uintptr_t)table % 16 || (uintptr_t)dst % 16 || (add && (uintptr_t)add % 16) ||
      (uintptr_t)idx % idx_bytes)
    return MCA_E_ALIGN;
  if (rows == 0) return MCA_OK;
  hipLaunchKernelGGL(embedding_mark_kernel, dim3(wave_grid((rows + 63) / 64)), dim3(256), 0, as_stream(stream), idx, idx_bytes, rows,
                     vocab, marker, flag, oob_bit);
  hipLaunchKernelGGL(embedding_renorm_marked_kernel, dim3(wave_grid((vocab + RENORM_CHUNK - 1) / RENORM_CHUNK)), dim3(256), 0, as_stream(stream),
                     table, vocab, cols, max_norm, marker);
  hipLaunchKernelGGL(embedding_gather_kernel, dim3(wave_grid(rows)), dim3(256), 0, as_stream(stream), table, vocab, cols, idx,
                     idx_bytes, rows, period, add, dst, ldd, dst_bstride, accumulate);
  return launch_status();
}

// =====================================================================================================
// table gradient
// =====================================================================================================
__device__ __forceinline__ const float* dy_row(const float* __restrict__ dy, int64_t ldy, int64_t y_bstride, int64_t period, int64_t i) {
  return dy + (i / period) * y_bstride + (i % period) * ldy;
}

// plain form: one wavefront per token, one atomic instruction per 64 consecutive floats (256 contiguous bytes of one row)
__global__ __launch_bounds__(256) void embedding_scatter_add_kernel(const float* __restrict__ dy, int64_t ldy, int64_t y_bstride,
                                                                     int64_t period, const void* __restrict__ idx, int idx_bytes,
                                                                     int64_t rows, float* __restrict__ dtable, int64_t vocab, int cols,
                                                                     int64_t padding_idx) {
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += (int64_t)gridDim.x * 4) {
    const int64_t v = token_row(idx, idx_bytes, i, vocab);
    if (v < 0 || v == padding_idx) continue;
    const float* g = dy_row(dy, ldy, y_bstride, period, i);
    float* d = dtable + v * cols;
    for (int c = lane; c < cols; c += 64) atomicAdd(d + c, g[c]);
  }
}

static int scatter_args_ok(const float* dy, int64_t period, const void* idx, int idx_bytes, int64_t rows, const float* dtable,
                           int64_t vocab, int cols) {
  if (!dy || !idx || !dtable || vocab <= 0 || cols <= 0 || rows < 0 || period <= 0) return MCA_E_BADARG;
  if (idx_bytes != 4 && idx_bytes != 8) return MCA_E_BADARG;
  if ((uintptr_t)idx % idx_bytes || (uintptr_t)dy % 4 || (uintptr_t)dtable % 4) return MCA_E_ALIGN;
  return MCA_OK;
}

extern "C" int mca_embedding_scatter_add(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period, const void* idx,
                                         int idx_bytes, int64_t rows, float* dtable, int64_t vocab, int cols, int64_t padding_idx,
                                         mca_stream_t stream) {
  const int rc = scatter_args_ok(dy, period, idx, idx_bytes, rows, dtable, vocab, cols);
  if (rc != MCA_OK || rows == 0) return rc;
  if (padding_idx < 0) padding_idx += vocab;
  hipLaunchKernelGGL(embedding_scatter_add_kernel, dim3(wave_grid(rows)), dim3(256), 0, as_stream(stream), dy, ldy, y_bstride, period,
                     idx, idx_bytes, rows, dtable, vocab, cols, padding_idx);
  return launch_status();
}

// ---- fixed-order form.  Launch 1 sorts the tokens by (table row, position): token i goes to place
//   #{ j : key_j < key_i  or  (key_j == key_i and j < i) },   key = its table row, or vocab when the token contributes nothing,
// counted directly (every thread walks all keys, a tile of 256 at a time through LDS): no atomics, every place written once.
// Launch 2: the wavefront that finds the first token of a table row at its place walks the row's tokens in that order.
__global__ __launch_bounds__(256) void embedding_sort_tokens_kernel(const void* __restrict__ idx, int idx_bytes, int64_t rows, int64_t vocab,
                                                                     int64_t padding_idx, int32_t* __restrict__ sorted_tok,
                                                                     int32_t* __restrict__ sorted_key) {
  __shared__ int32_t tile[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int32_t key = 0;
  if (i < rows) {
    const int64_t v = token_row(idx, idx_bytes, i, vocab);
    key = (int32_t)((v < 0 || v == padding_idx) ? vocab : v);
  }
  int64_t place = 0;
  for (int64_t j0 = 0; j0 < rows; j0 += 256) {
    const int64_t j = j0 + threadIdx.x;
    int32_t kj = 0;
    if (j < rows) {
      const int64_t v = token_row(idx, idx_bytes, j, vocab);
      kj = (int32_t)((v < 0 || v == padding_idx) ? vocab : v);
    }
    __syncthreads();
    tile[threadIdx.x] = kj;
    __syncthreads();
    const int n = rows - j0 < 256 ? (int)(rows - j0) : 256;
    for (int t = 0; t < n; t++) {
      const int32_t k = tile[t];
      place += (k < key) | ((k == key) & (j0 + t < i));
    }
  }
  if (i < rows) { sorted_tok[place] = (int32_t)i; sorted_key[place] = key; }
}

__global__ __launch_bounds__(256) void embedding_sum_sorted_kernel(const float* __restrict__ dy, int64_t ldy, int64_t y_bstride,
                                                                    int64_t period, const int32_t* __restrict__ sorted_tok,
                                                                    const int32_t* __restrict__ sorted_key, int64_t rows,
                                                                    float* __restrict__ dtable, int64_t vocab, int cols) {
  const int lane = threadIdx.x & 63, chunks = (cols + 63) / 64;
  const int64_t items = rows * chunks;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < items; w += (int64_t)gridDim.x * 4) {
    const int64_t p = w / chunks;
    const int c = (int)(w % chunks) * 64 + lane;
    const int32_t key = sorted_key[p];
    if (key >= vocab || (p > 0 && sorted_key[p - 1] == key)) continue;          // no contribution | not the row's first token
    float acc = 0.f;
    for (int64_t q = p; q < rows && sorted_key[q] == key; q++) {
      const float* g = dy_row(dy, ldy, y_bstride, period, sorted_tok[q]);
      if (c < cols) acc += g[c];
    }
    if (c < cols) dtable[(int64_t)key * cols + c] += acc;
  }
}

extern "C" int64_t mca_embedding_scatter_add_det_scratch(int64_t rows) { return rows > 0 ? 2 * rows : 0; }

extern "C" int mca_embedding_scatter_add_det(const float* dy, int64_t ldy, int64_t y_bstride, int64_t period, const void* idx,
                                             int idx_bytes, int64_t rows, float* dtable, int64_t vocab, int cols, int64_t padding_idx,
                                             float* scratch, int64_t scratch_floats, mca_stream_t stream) {
  const int rc = scatter_args_ok(dy, period, idx, idx_bytes, rows, dtable, vocab, cols);
  if (rc != MCA_OK || rows == 0) return rc;
  if (rows >= (int64_t)1 << 31 || vocab >= (int64_t)1 << 31) return MCA_E_UNSUPPORTED;          // places and keys are 32-bit
  if (!scratch || scratch_floats < 2 * rows) return MCA_E_BADARG;
  if (padding_idx < 0) padding_idx += vocab;
  int32_t* sorted_tok = reinterpret_cast<int32_t*>(scratch);
  int32_t* sorted_key = sorted_tok + rows;
  hipLaunchKernelGGL(embedding_sort_tokens_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, as_stream(stream), idx, idx_bytes,
                     rows, vocab, padding_idx, sorted_tok, sorted_key);
  hipLaunchKernelGGL(embedding_sum_sorted_kernel, dim3(wave_grid(rows * ((cols + 63) / 64))), dim3(256), 0, as_stream(stream), dy, ldy,
                     y_bstride, period, sorted_tok, sorted_key, rows, dtable, vocab, cols);
  return launch_status();
}
