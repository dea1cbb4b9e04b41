// Supervised task head over the pooled tokens (include/mca_hip.h, mca_task_head_fwd_bwd): a linear head on ONE slot of the
// (b, R, D) pooled tokens, an elementwise loss against a window of a label matrix, the head's gradients and the gradient with
// respect to the pooled tokens added onto a scaled base (the contrastive loss's d_pooled).  Two launches, no atomics:
//   rows kernel      one workgroup per block of TH_ROWS rows, one wave per row: logits, pred, element loss, dz, d_pooled; then the
//                    workgroup's share of gw / gb (rows in order) and of the loss go to its slot of the workspace;
//   finalize kernel  adds the slots in block order into gw, gb and the loss.
// Every workgroup counts the valid rows itself (an integer count: exact in any order), so dz needs no third launch.
#include "common.h"

namespace {

constexpr int TH_ROWS = 64;          // rows per workgroup (include/mca_hip.h: the workspace is sized by it)
constexpr int TH_MAX_D = 1024, TH_MAX_L = 64;

__host__ __device__ inline int64_t th_slot_floats(int L, int D) { return (int64_t)L * D + ((L + 3) & ~3) + 4; }

__device__ __forceinline__ bool th_valid(const uint32_t* __restrict__ present, uint32_t any_bits, int64_t s) {
  return any_bits == 0 || (present[s] & any_bits) != 0;
}

__device__ __forceinline__ float4 fma4(float a, float4 x, float4 c) {
  return make_float4(fmaf(a, x.x, c.x), fmaf(a, x.y, c.y), fmaf(a, x.z, c.z), fmaf(a, x.w, c.w));
}

__global__ __launch_bounds__(256) void task_head_rows_kernel(mca_task_head_args A) {
  __shared__ float dzs[TH_ROWS][TH_MAX_L];
  __shared__ float red[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = A.b, R = A.R, D = A.D, L = A.L, D4 = D >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * TH_ROWS;
  const int nrows = (int)(b - r0 < TH_ROWS ? b - r0 : TH_ROWS);

  // n_valid, by every workgroup for itself
  int cnt = 0;
  for (int64_t s = tid; s < b; s += 256) cnt += th_valid(A.present, A.any_bits, s) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, WAVE);
  if (lane == 0) redi[wv] = cnt;
  __syncthreads();
  const int n_valid = redi[0] + redi[1] + redi[2] + redi[3];
  const float scale = n_valid > 0 ? A.task_weight / ((float)n_valid * (float)L) : 0.f;          // task_weight / n
  const float base = A.d_pooled_in ? A.base_weight : 0.f;

  float loss_w = 0.f;          // this wave's rows, in order
  for (int i = wv; i < nrows; i += 4) {
    const int64_t s = r0 + i;
    const bool valid = th_valid(A.present, A.any_bits, s);
    const float4* x4 = reinterpret_cast<const float4*>(A.pooled + (s * R + A.slot) * D);
    float4 xv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) xv[j] = (lane + 64 * j < D4) ? x4[lane + 64 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
    float my_z = 0.f;
    for (int l = 0; l < L; l++) {
      const float4* w4 = reinterpret_cast<const float4*>(A.w + (int64_t)l * D);
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (lane + 64 * j < D4) {
          const float4 wj = w4[lane + 64 * j];
          acc = fmaf(xv[j].x, wj.x, acc); acc = fmaf(xv[j].y, wj.y, acc); acc = fmaf(xv[j].z, wj.z, acc); acc = fmaf(xv[j].w, wj.w, acc);
        }
      acc = wave_sum(acc) + A.bias[l];
      if (lane == l) my_z = acc;
    }
    float dz = 0.f, le = 0.f;
    if (lane < L) {
      A.pred[s * L + lane] = my_z;
      if (valid) {
        const float z = my_z, yv = A.labels[s * A.ld_labels + lane], e = z - yv;
        float g;
        if (A.loss_type == 0) {          // L1, sign(0) = 0
          le = fabsf(e);
          g = (float)((e > 0.f) - (e < 0.f));
        } else if (A.loss_type == 1) {   // MSE
          le = e * e;
          g = 2.f * e;
        } else {                         // BCE with logits
          le = fmaxf(z, 0.f) - z * yv + log1pf(expf(-fabsf(z)));
          g = 1.f / (1.f + expf(-z)) - yv;
        }
        dz = g * scale;
      }
      dzs[i][lane] = dz;
    }
    loss_w += wave_sum(le);
    // d_pooled[s, r, :] = base * d_pooled_in[s, r, :] + (r == slot ? sum_l dz[l] w[l, :] : 0)
    float4 dx[4];
#pragma unroll
    for (int j = 0; j < 4; j++) dx[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < L; l++) {
      const float gl = __shfl(dz, l, WAVE);
      const float4* w4 = reinterpret_cast<const float4*>(A.w + (int64_t)l * D);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (lane + 64 * j < D4) dx[j] = fma4(gl, w4[lane + 64 * j], dx[j]);
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
  float* part = A.workspace + (int64_t)blockIdx.x * th_slot_floats(L, D);
  const float* xs = A.pooled + (r0 * R + A.slot) * D;
  const int64_t xstride = (int64_t)R * D;
  for (int it = tid; it < L * D4; it += 256) {
    const int l = it / D4, k4 = it - l * D4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = 0; i < nrows; i++) acc = fma4(dzs[i][l], reinterpret_cast<const float4*>(xs + i * xstride)[k4], acc);
    reinterpret_cast<float4*>(part)[it] = acc;
  }
  float* tail = part + (int64_t)L * D;
  const int Lp = (L + 3) & ~3;
  if (tid < Lp) {
    float acc = 0.f;
    if (tid < L)
      for (int i = 0; i < nrows; i++) acc += dzs[i][tid];
    tail[tid] = acc;
  }
  if (tid == 0) {
    tail[Lp] = (red[0] + red[1]) + (red[2] + red[3]);
    tail[Lp + 1] = (float)n_valid;
    tail[Lp + 2] = 0.f;
    tail[Lp + 3] = 0.f;
  }
}

// gw, gb (+)= the slots in block order; loss[0] = (sum of the slots' losses) / (n_valid L), loss[1] = n_valid
__global__ __launch_bounds__(256) void task_head_final_kernel(const float* __restrict__ ws, int nblk, int L, int D, int accumulate,
                                                              float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ loss) {
  const int64_t stride = th_slot_floats(L, D);
  const int n4 = L * (D >> 2), Lp = (L + 3) & ~3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < n4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < nblk; c++) {
      const float4 v = reinterpret_cast<const float4*>(ws + c * stride)[t];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4* o = reinterpret_cast<float4*>(gw) + t;
    if (accumulate) {
      const float4 old = *o;
      acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w;
    }
    *o = acc;
  } else if (t < n4 + L) {
    const int l = t - n4;
    float acc = 0.f;
    for (int c = 0; c < nblk; c++) acc += ws[c * stride + (int64_t)L * D + l];
    gb[l] = accumulate ? gb[l] + acc : acc;
  } else if (t == n4 + L) {
    float acc = 0.f;
    for (int c = 0; c < nblk; c++) acc += ws[c * stride + (int64_t)L * D + Lp];
    const float nv = ws[(int64_t)L * D + Lp + 1];
    loss[0] = nv > 0.f ? acc / (nv * (float)L) : 0.f;
    loss[1] = nv;
  }
}

}  // namespace

extern "C" int64_t mca_task_head_workspace_bytes(int b, int L, int D) {
  if (b < 1 || L < 1 || L > TH_MAX_L || D < 4 || D > TH_MAX_D || D % 4) return -1;
  return (((int64_t)b + TH_ROWS - 1) / TH_ROWS) * th_slot_floats(L, D) * (int64_t)sizeof(float);
}

extern "C" int mca_task_head_fwd_bwd(const mca_task_head_args* args, mca_stream_t stream) {
  if (!args) return MCA_E_BADARG;
  const mca_task_head_args& a = *args;
  if (!a.pooled || !a.w || !a.bias || !a.labels || !a.pred || !a.loss || !a.d_pooled || !a.gw || !a.gb || !a.workspace) return MCA_E_BADARG;
  if (a.b < 1 || a.R < 1 || a.D < 1 || a.L < 1) return MCA_E_BADARG;
  if (a.D > TH_MAX_D || a.L > TH_MAX_L) return MCA_E_UNSUPPORTED;
  if (a.slot < 0 || a.slot >= a.R || a.ld_labels < a.L) return MCA_E_BADARG;
  if (a.loss_type < 0 || a.loss_type > 2 || (a.accumulate != 0 && a.accumulate != 1)) return MCA_E_BADARG;
  if (a.any_bits != 0 && !a.present) return MCA_E_BADARG;
  if (!(a.task_weight == a.task_weight) || !(a.base_weight == a.base_weight)) return MCA_E_BADARG;          // NaN weights
  if (a.D % 4) return MCA_E_ALIGN;
  if (a.workspace_bytes < mca_task_head_workspace_bytes(a.b, a.L, a.D)) return MCA_E_BADARG;
  const uintptr_t wide = (uintptr_t)a.pooled | (uintptr_t)a.w | (uintptr_t)a.d_pooled | (uintptr_t)a.d_pooled_in | (uintptr_t)a.gw |
                         (uintptr_t)a.workspace;
  const uintptr_t narrow = (uintptr_t)a.bias | (uintptr_t)a.labels | (uintptr_t)a.pred | (uintptr_t)a.loss | (uintptr_t)a.gb |
                           (uintptr_t)a.present;
  if (wide % 16 || narrow % 4) return MCA_E_ALIGN;
  const int nblk = (a.b + TH_ROWS - 1) / TH_ROWS;
  hipLaunchKernelGGL(task_head_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, as_stream(stream), a);
  const int items = a.L * (a.D / 4) + a.L + 1;
  hipLaunchKernelGGL(task_head_final_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, as_stream(stream), a.workspace, nblk, a.L,
                     a.D, a.accumulate, a.gw, a.gb, a.loss);
  return launch_status();
}
