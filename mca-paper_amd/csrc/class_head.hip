// Softmax cross-entropy heads over class-index labels (include/mca_hip.h): the classification twins of the probe head
// (mca_probe_head_f32, evaluate.hip) and of the task head (mca_task_head_fwd_bwd, task_head.hip).  Both give one wavefront a row
// and one lane a class (C <= 64): the row maximum, the sum of exponentials and every dot product are wave reductions over a fixed xor
// tree, the maximum is subtracted before expf and the row loss is (m + logf(S)) - z_y.  No atomics: two calls give the same bits.
//   mca_probe_head_ce_f32    one launch, four rows a workgroup, loss_part[block] = the block's sum of row losses
//   mca_class_head_fwd_bwd   rows kernel (64 rows a workgroup: logits, pred, row loss, dz, d_pooled, then the workgroup's share of
//                            gw / gb / loss into its workspace slot, rows in order) and a finalize that adds the slots in block order.
// Every workgroup of the rows kernel forms the divisor W = sum of class_weights[y_s] over the counted rows itself, all of them by
// the same fixed order, so dz needs no third launch.
#include "common.h"

namespace {

constexpr int CH_ROWS = 64;          // rows per workgroup (include/mca_hip.h: the workspace is sized by it)
constexpr int CH_MAX_D = 1024, CH_MAX_C = 64;

__host__ __device__ inline int64_t ch_slot_floats(int C, int D) { return (int64_t)C * D + ((C + 3) & ~3) + 4; }

__device__ __forceinline__ float4 ch_fma4(float a, float4 x, float4 c) {
  return make_float4(fmaf(a, x.x, c.x), fmaf(a, x.y, c.y), fmaf(a, x.z, c.z), fmaf(a, x.w, c.w));
}

// a label is a class index iff it is an integer value in [0, C); NaN fails every comparison.  -1 when it is none.
__device__ __forceinline__ int ch_class_of(float y, int C) {
  return (y >= 0.f && y < (float)C && y == floorf(y)) ? (int)y : -1;
}

// the class of row s, or -1 when the row is not counted; the label of a row that is invalid by presence is not read
__device__ __forceinline__ int ch_row_class(const mca_class_head_args& A, int64_t s) {
  if (A.any_bits != 0 && (A.present[s] & A.any_bits) == 0) return -1;
  return ch_class_of(A.labels[s * A.ld_labels], A.C);
}

// softmax statistics of one row held one logit per lane (lanes >= C idle): p = softmax(z)[lane], lse = m + logf(S)
__device__ __forceinline__ void ch_softmax(float z, bool live, float& p, float& lse) {
  const float m = wave_max(live ? z : -INFINITY);
  const float e = live ? expf(z - m) : 0.f;
  const float S = wave_sum(e);
  p = e / S;
  lse = m + logf(S);
}

__global__ __launch_bounds__(256) void probe_head_ce_kernel(const float* __restrict__ a, int64_t lda, const int32_t* __restrict__ aidx, int K,
                                                            const float* __restrict__ w, const float* __restrict__ bias, int C,
                                                            const float* __restrict__ labels, int64_t ldy, const int32_t* __restrict__ yidx,
                                                            int64_t B, float inv_count, float* __restrict__ pred, float* __restrict__ dz,
                                                            float* __restrict__ da, float dact_scale, float* __restrict__ loss_part) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  float loss_r = 0.f;
  if (row < B) {
    const int64_t src = aidx ? aidx[row] : row;
    float av[16];
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = (j * 64 + lane < K) ? a[src * lda + j * 64 + lane] : 0.f;
    float my_z = 0.f;
    for (int c = 0; c < C; c++) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++)
        if (j * 64 + lane < K) s = fmaf(av[j], w[(int64_t)c * K + j * 64 + lane], s);
      s = wave_sum(s) + bias[c];
      if (lane == c) my_z = s;
    }
    const bool live = lane < C;
    float p, lse;
    ch_softmax(my_z, live, p, lse);
    const int y = ch_class_of(labels[(int64_t)(yidx ? yidx[row] : row) * ldy], C);
    float g = 0.f;
    if (y >= 0) {
      loss_r = lse - __shfl(my_z, y, WAVE);
      if (live) g = (p - (lane == y ? 1.f : 0.f)) * inv_count;
    }
    if (live) {
      pred[row * C + lane] = my_z;
      if (dz) dz[row * C + lane] = g;
    }
    if (da) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int k = j * 64 + lane;
        float s = 0.f;
        for (int c = 0; c < C; c++) {
          const float gc = __shfl(g, c, WAVE);
          if (k < K) s = fmaf(gc, w[(int64_t)c * K + k], s);
        }
        if (k < K) da[row * K + k] = av[j] > 0.f ? s * dact_scale : 0.f;
      }
    }
  }
  if (lane == 0) red[wv] = loss_r;          // the row loss is the same in every lane
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void class_head_rows_kernel(mca_class_head_args A) {
  __shared__ float dzs[CH_ROWS][CH_MAX_C];
  __shared__ float red[4];
  __shared__ float redw[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = A.b, R = A.R, D = A.D, C = A.C, D4 = D >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * CH_ROWS;
  const int nrows = (int)(b - r0 < CH_ROWS ? b - r0 : CH_ROWS);
  const bool live = lane < C;
  const float cw = live ? (A.class_weights ? A.class_weights[lane] : 1.f) : 0.f;
  const float cw_sum = wave_sum(cw);

  // the counted rows and W, by every workgroup for itself and by all of them in the same order
  int cnt = 0;
  float wsum = 0.f;
  for (int64_t s = tid; s < b; s += 256) {
    const int y = ch_row_class(A, s);
    if (y >= 0) {
      cnt += 1;
      wsum += A.class_weights ? A.class_weights[y] : 1.f;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, WAVE);
  wsum = wave_sum(wsum);
  if (lane == 0) {
    redi[wv] = cnt;
    redw[wv] = wsum;
  }
  __syncthreads();
  const int n_counted = redi[0] + redi[1] + redi[2] + redi[3];
  const float W = (redw[0] + redw[1]) + (redw[2] + redw[3]);
  const float scale = W > 0.f ? A.task_weight / W : 0.f;
  const float base = A.d_pooled_in ? A.base_weight : 0.f;
  const float hard = 1.f - A.label_smoothing, soft = A.label_smoothing / (float)C;

  float loss_w = 0.f;          // this wave's rows, in order
  for (int i = wv; i < nrows; i += 4) {
    const int64_t s = r0 + i;
    const int y = ch_row_class(A, s);
    const float4* x4 = reinterpret_cast<const float4*>(A.pooled + (s * R + A.slot) * D);
    float4 xv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) xv[j] = (lane + 64 * j < D4) ? x4[lane + 64 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
    float my_z = 0.f;
    for (int c = 0; c < C; c++) {
      const float4* w4 = reinterpret_cast<const float4*>(A.w + (int64_t)c * D);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (lane + 64 * j < D4) {
          const float4 wj = w4[lane + 64 * j];
          acc = fmaf(xv[j].x, wj.x, acc); acc = fmaf(xv[j].y, wj.y, acc); acc = fmaf(xv[j].z, wj.z, acc); acc = fmaf(xv[j].w, wj.w, acc);
        }
      acc = wave_sum(acc) + A.bias[c];
      if (lane == c) my_z = acc;
    }
    float dz = 0.f;
    if (live) A.pred[s * C + lane] = my_z;
    if (y >= 0) {          // wave-uniform
      float p, lse;
      ch_softmax(my_z, live, p, lse);
      const float cwy = __shfl(cw, y, WAVE);
      const float nll = lse - __shfl(my_z, y, WAVE);
      float row_loss = hard * cwy * nll;
      dz = hard * cwy * (p - (lane == y ? 1.f : 0.f));
      if (A.label_smoothing > 0.f) {
        row_loss += soft * wave_sum(live ? cw * (lse - my_z) : 0.f);
        dz += soft * (p * cw_sum - cw);
      }
      dz = live ? dz * scale : 0.f;
      loss_w += row_loss;
    }
    if (live) dzs[i][lane] = dz;
    // d_pooled[s, r, :] = base * d_pooled_in[s, r, :] + (r == slot ? sum_c dz[c] w[c, :] : 0)
    float4 dx[4];
#pragma unroll
    for (int j = 0; j < 4; j++) dx[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < C; c++) {
      const float gc = __shfl(dz, c, WAVE);
      const float4* w4 = reinterpret_cast<const float4*>(A.w + (int64_t)c * D);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (lane + 64 * j < D4) dx[j] = ch_fma4(gc, w4[lane + 64 * j], dx[j]);
    }
    for (int r = 0; r < R; r++) {
      const int64_t row = (s * R + r) * D;
      float4* out4 = reinterpret_cast<float4*>(A.d_pooled + row);
      const float4* in4 = A.d_pooled_in ? reinterpret_cast<const float4*>(A.d_pooled_in + row) : nullptr;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (lane + 64 * j < D4) {
          const float4 din = in4 ? in4[lane + 64 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 add = r == A.slot ? dx[j] : make_float4(0.f, 0.f, 0.f, 0.f);
          out4[lane + 64 * j] = make_float4(fmaf(base, din.x, add.x), fmaf(base, din.y, add.y), fmaf(base, din.z, add.z), fmaf(base, din.w, add.w));
        }
    }
  }
  if (lane == 0) red[wv] = loss_w;
  __syncthreads();          // dzs and red are complete

  // the workgroup's share of gw, gb and the loss: rows in order
  float* part = A.workspace + (int64_t)blockIdx.x * ch_slot_floats(C, D);
  const float* xs = A.pooled + (r0 * R + A.slot) * D;
  const int64_t xstride = (int64_t)R * D;
  for (int it = tid; it < C * D4; it += 256) {
    const int c = it / D4, k4 = it - c * D4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < nrows; i++) acc = ch_fma4(dzs[i][c], reinterpret_cast<const float4*>(xs + i * xstride)[k4], acc);
    reinterpret_cast<float4*>(part)[it] = acc;
  }
  float* tail = part + (int64_t)C * D;
  const int Cp = (C + 3) & ~3;
  if (tid < Cp) {
    float acc = 0.f;
    if (tid < C)
      for (int i = 0; i < nrows; i++) acc += dzs[i][tid];
    tail[tid] = acc;
  }
  if (tid == 0) {
    tail[Cp] = (red[0] + red[1]) + (red[2] + red[3]);
    tail[Cp + 1] = (float)n_counted;
    tail[Cp + 2] = W;
    tail[Cp + 3] = 0.f;
  }
}

// gw, gb (+)= the slots in block order; loss[0] = (sum of the slots' losses) / W, loss[1] = the counted rows, loss[2] = W
__global__ __launch_bounds__(256) void class_head_final_kernel(const float* __restrict__ ws, int nblk, int C, int D, int accumulate,
                                                               float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ loss) {
  const int64_t stride = ch_slot_floats(C, D);
  const int n4 = C * (D >> 2), Cp = (C + 3) & ~3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < n4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < nblk; k++) {
      const float4 v = reinterpret_cast<const float4*>(ws + k * stride)[t];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4* o = reinterpret_cast<float4*>(gw) + t;
    if (accumulate) {
      const float4 old = *o;
      acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w;
    }
    *o = acc;
  } else if (t < n4 + C) {
    const int c = t - n4;
    float acc = 0.f;
    for (int k = 0; k < nblk; k++) acc += ws[k * stride + (int64_t)C * D + c];
    gb[c] = accumulate ? gb[c] + acc : acc;
  } else if (t == n4 + C) {
    float acc = 0.f;
    for (int k = 0; k < nblk; k++) acc += ws[k * stride + (int64_t)C * D + Cp];
    const float W = ws[(int64_t)C * D + Cp + 2];
    loss[0] = W > 0.f ? acc / W : 0.f;
    loss[1] = ws[(int64_t)C * D + Cp + 1];
    loss[2] = W;
  }
}

}  // namespace

extern "C" int mca_probe_head_ce_f32(const float* a, int64_t lda, const int32_t* aidx, int64_t K, const float* w, const float* bias, int64_t C,
                                     const float* labels, int64_t ldy, const int32_t* yidx, int64_t B, float* pred, float* dz, float* da,
                                     float dact_scale, float* loss_part, mca_stream_t stream) {
  if (!a || !w || !bias || !labels || !pred || !loss_part || B <= 0 || K <= 0 || C < 2 || lda < K || ldy < 1) return MCA_E_BADARG;
  if (K > 1024 || C > CH_MAX_C) return MCA_E_UNSUPPORTED;
  hipLaunchKernelGGL(probe_head_ce_kernel, dim3((unsigned)mca_probe_head_blocks(B)), dim3(256), 0, as_stream(stream), a, lda, aidx, (int)K, w,
                     bias, (int)C, labels, ldy, yidx, B, 1.f / (float)B, pred, dz, da, dact_scale, loss_part);
  return launch_status();
}

extern "C" int64_t mca_class_head_workspace_bytes(int b, int C, int D) {
  if (b < 1 || C < 2 || C > CH_MAX_C || D < 4 || D > CH_MAX_D || D % 4) return -1;
  return (((int64_t)b + CH_ROWS - 1) / CH_ROWS) * ch_slot_floats(C, D) * (int64_t)sizeof(float);
}

extern "C" int mca_class_head_fwd_bwd(const mca_class_head_args* args, mca_stream_t stream) {
  if (!args) return MCA_E_BADARG;
  const mca_class_head_args& a = *args;
  if (!a.pooled || !a.w || !a.bias || !a.labels || !a.pred || !a.loss || !a.d_pooled || !a.gw || !a.gb || !a.workspace) return MCA_E_BADARG;
  if (a.b < 1 || a.R < 1 || a.D < 1 || a.C < 2) return MCA_E_BADARG;
  if (a.D > CH_MAX_D || a.C > CH_MAX_C) return MCA_E_UNSUPPORTED;
  if (a.slot < 0 || a.slot >= a.R || a.ld_labels < 1) return MCA_E_BADARG;
  if (!(a.label_smoothing >= 0.f && a.label_smoothing < 1.f) || (a.accumulate != 0 && a.accumulate != 1)) return MCA_E_BADARG;          // NaN too
  if (a.any_bits != 0 && !a.present) return MCA_E_BADARG;
  if (!(a.task_weight == a.task_weight) || !(a.base_weight == a.base_weight)) return MCA_E_BADARG;          // NaN weights
  if (a.D % 4) return MCA_E_ALIGN;
  if (a.workspace_bytes < mca_class_head_workspace_bytes(a.b, a.C, a.D)) return MCA_E_BADARG;
  const uintptr_t wide = (uintptr_t)a.pooled | (uintptr_t)a.w | (uintptr_t)a.d_pooled | (uintptr_t)a.d_pooled_in | (uintptr_t)a.gw |
                         (uintptr_t)a.workspace;
  const uintptr_t narrow = (uintptr_t)a.bias | (uintptr_t)a.labels | (uintptr_t)a.class_weights | (uintptr_t)a.pred | (uintptr_t)a.loss |
                           (uintptr_t)a.gb | (uintptr_t)a.present;
  if (wide % 16 || narrow % 4) return MCA_E_ALIGN;
  const int nblk = (a.b + CH_ROWS - 1) / CH_ROWS;
  hipLaunchKernelGGL(class_head_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), a);
  const int items = a.C * (a.D / 4) + a.C + 1;
  hipLaunchKernelGGL(class_head_final_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, as_stream(stream), a.workspace, nblk, a.C,
                     a.D, a.accumulate, a.gw, a.gb, a.loss);
  return launch_status();
}
