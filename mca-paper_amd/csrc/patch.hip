// PatchEncoder front end (reference encoders.py:247-251,260-262,273, mode "matrix"): one pass over a (b, H, W) fp32 matrix batch
// that gathers the (p1, p2) patches into token rows, applies the first LayerNorm(P), writes the bf16 GEMM operand and derives the
// key-padding mask (a patch is padded when EVERY element equals pad_value).  mca_patch_nd_ln_fwd, further down, is the same pass over
// a (b, C, T, H, W) batch in (pt, p1, p2) patches (ImagePatchEncoder, VideoPatchEncoder; the reference's :252-259 with the grid merged).
//
// Bandwidth-bound: values is read once; xp (same size), xn_bf16 (half) and three small vectors are written.  A patch row is only
// p2 contiguous floats (64 B at p2 = 16), so a wavefront that reads its patch straight from global memory issues short segments.
// Staged form instead: a workgroup takes the strip of p1 matrix rows under a span of S patches of one patch row, reads whole
// strip rows (S * p2 contiguous floats) coalesced, and stores them into LDS in PATCH order.  Each wavefront then normalises whole
// patches out of LDS and writes its rows of xp / xn_bf16 as contiguous segments.
//
// LDS layout: patch j of the span starts at j * PS floats, element (r, c) of it at r * p2 + c.  PS is the smallest value >= P with
// PS % 64 == p2 % 64.  The staging store of strip element (r, cc = j * p2 + c) then lands in bank (cc + r * p2) mod 64: lanes
// that walk along a strip row hit consecutive banks whatever p2 is (p2 = 16: 16-lane groups 16 banks apart; p2 = 1: one bank per
// lane).  The normalising read of a patch is contiguous in LDS, so it has no conflicts either.
//
// Statistics as the LayerNorm kernels of elementwise.hip: two passes (mean, then centred squares), at most 16 sequential adds per
// lane followed by the 6 shuffle levels of wave_sum, so the bounds derived for those kernels (docs/parity.md, "Row and streaming
// kernels") hold here unchanged.
#include "common.h"

#define PATCH_MAX_P 1024           // 16 elements per lane of one wavefront
#define PATCH_MAX_SPAN 64          // patches per workgroup
#define PATCH_LDS_FLOATS 8192      // >= span * PS for every span patch_span() returns (span * P <= 4096, span * 63 <= 4032)

static inline int patch_span(int P, int npw) {
  int s = 4096 / P;                // P = 1024: one patch per wavefront of the workgroup
  if (s > PATCH_MAX_SPAN) s = PATCH_MAX_SPAN;
  const int cap = mca_knobs[13] < 0 ? -mca_knobs[13] : mca_knobs[13];          // knob 13 = +-c: at most c patches per workgroup (A/B)
  if (cap > 0 && s > cap) s = cap;
  return s < npw ? s : npw;
}
// The N-D kernel's span: the budget rounded down to a power of two before the row caps it.  A budget such as 5 (P = 768) or 10
// (P = 384) patches leaves the staging grid, whose width is a power of two, with idle column lanes and gives the four wavefronts an
// uneven share of patches: measured 19.8 against 16.0 us and 46.0 against 34.1 us (profiles/patch_nd_encoder.md).
static inline int patch_nd_span(int P, int npw) {
  int s = patch_span(P, 0x7fffffff);
  while (s & (s - 1)) s &= s - 1;
  return s < npw ? s : npw;
}
static inline int patch_stride(int P, int p2) { return P + ((p2 - P) % 64 + 64) % 64; }

// The normalising stage, shared by both kernels: one wavefront, one patch.  at(c) is the address of element c of the patch (VEC
// consecutive elements from there are contiguous).  Two-pass statistics, the exact values of an all-pad patch, then the stores of
// mean / rstd / padmask, xp (optional) and xn with its zero columns [P, cols_pad).
template <int VEC, typename At>
__device__ __forceinline__ void patch_normalise(At at, int P, int lane, int64_t row, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float pad_value, float eps, float* __restrict__ xp,
                                                u16* __restrict__ xn, int64_t ld_bf16, int cols_pad, float* __restrict__ mean_out,
                                                float* __restrict__ rstd_out, uint8_t* __restrict__ padmask) {
  constexpr int NI = 16 / VEC;
  float v[NI][VEC];
  float sum = 0.f;
  bool pad = true;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int c = (lane + 64 * i) * VEC;
    if (c < P) {
      const float* pe = at(c);
      if (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(pe);
        v[i][0] = t.x; v[i][1 % VEC] = t.y; v[i][2 % VEC] = t.z; v[i][3 % VEC] = t.w;
      } else {
        v[i][0] = pe[0];
      }
#pragma unroll
      for (int k = 0; k < VEC; k++) { sum += v[i][k]; pad = pad && (v[i][k] == pad_value); }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; k++) v[i][k] = 0.f;
    }
  }
  pad = __all(pad);
  float mean = wave_sum(sum) / (float)P;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    if ((lane + 64 * i) * VEC < P) {
#pragma unroll
      for (int k = 0; k < VEC; k++) { const float d = v[i][k] - mean; q += d * d; }
    }
  }
  float rstd = rsqrtf(wave_sum(q) / (float)P + eps);
  if (pad) { mean = pad_value; rstd = rsqrtf(eps); }          // the exact statistics of a constant row
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; padmask[row] = pad ? 1 : 0; }
  float* xr = xp ? xp + row * (int64_t)P : nullptr;
  u16* br = xn + row * ld_bf16;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int c = (lane + 64 * i) * VEC;
    if (c < P) {
      float o[VEC];
#pragma unroll
      for (int k = 0; k < VEC; k++) o[k] = pad ? beta[c + k] : (v[i][k] - mean) * rstd * gamma[c + k] + beta[c + k];
      if (VEC == 4) {
        uint2 pk; pk.x = pack2bf(o[0], o[1 % VEC]); pk.y = pack2bf(o[2 % VEC], o[3 % VEC]);
        *reinterpret_cast<uint2*>(br + c) = pk;
        if (xr) *reinterpret_cast<float4*>(xr + c) = make_float4(v[i][0], v[i][1 % VEC], v[i][2 % VEC], v[i][3 % VEC]);
      } else {
        br[c] = f2bf(o[0]);
        if (xr) xr[c] = v[i][0];
      }
    }
  }
  for (int c = P + lane; c < cols_pad; c += 64) br[c] = 0;
}

// VEC = 4: every global and LDS access of four consecutive elements is one 16-byte (bf16: 8-byte) access; the host picks it when
// p2 % 4 == 0 and every base and stride is aligned.  tw_log2: the workgroup's 256 threads form a (256 >> tw_log2) x (1 << tw_log2)
// grid over (strip row, VEC-column group), so that a narrow strip (W = 128: 32 float4 per row) still keeps every thread loading.
// DIRECT (A/B knob 13 < 0, tools/bench_patch_encoder.py): the wavefront-per-patch form without the staging: each wavefront reads its
// patch from global memory, p2 contiguous floats per patch row; same arithmetic, same stores, no LDS and no barrier.
template <int VEC, bool DIRECT>
__global__ __launch_bounds__(256) void patch_ln_fwd_kernel(
    const float* __restrict__ values, int64_t v_bstride, int64_t ldv, int gh, int npw, int p1, int p2, int span, int n_span, int ps,
    int tw_log2, const float* __restrict__ gamma, const float* __restrict__ beta, float pad_value, float eps,
    float* __restrict__ xp, u16* __restrict__ xn, int64_t ld_bf16, int cols_pad,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, uint8_t* __restrict__ padmask) {
  extern __shared__ __align__(16) float strip[];
  const int P = p1 * p2;
  int bid = blockIdx.x;
  const int sp = bid % n_span; bid /= n_span;
  const int pi = bid % gh;
  const int s = bid / gh;
  const int j0 = sp * span;
  const int cur = min(span, npw - j0);          // patches of this workgroup
  const int sw = cur * p2;                      // floats per strip row
  const float* src = values + (int64_t)s * v_bstride + (int64_t)pi * p1 * ldv + (int64_t)j0 * p2;          // the strip's first element
  // ---- stage: strip rows, coalesced, into patch order
  if (!DIRECT) {
    const int tx = threadIdx.x & ((1 << tw_log2) - 1), ty = threadIdx.x >> tw_log2, th = 256 >> tw_log2;
    for (int cc = tx * VEC; cc < sw; cc += VEC << tw_log2) {
      const int j = cc / p2, c = cc - j * p2;          // (VEC = 4: p2 % 4 == 0, the four elements are of one patch row)
      float* dst = strip + j * ps + c;
      for (int r = ty; r < p1; r += th) {
        if (VEC == 4) *reinterpret_cast<float4*>(dst + r * p2) = *reinterpret_cast<const float4*>(src + (int64_t)r * ldv + cc);
        else dst[r * p2] = src[(int64_t)r * ldv + cc];
      }
    }
    __syncthreads();
  }
  // ---- normalise: one wavefront per patch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < cur; j += 4) {
    const int64_t row = ((int64_t)s * gh + pi) * npw + j0 + j;
    const float* pr = strip + j * ps;
    patch_normalise<VEC>([&](int c) -> const float* {
      if (DIRECT) { const int r = c / p2; return src + (int64_t)r * ldv + j * p2 + (c - r * p2); }
      return pr + c;
    }, P, lane, row, gamma, beta, pad_value, eps, xp, xn, ld_bf16, cols_pad, mean_out, rstd_out, padmask);
  }
}

// The N-D form: values is a (b, C, T, H, W) batch with explicit batch, channel, frame and row strides, cut into (pt, p1, p2) patches;
// a patch is R = C * pt * p1 runs of p2 contiguous floats spread over planes and frames.  Same staging: a workgroup takes a span of
// patches along W of one (sample, ti, hi) and reads each of the R strip rows (c, dt, r) as one coalesced run of span * p2 floats;
// strip row q = (c * pt + dt) * p1 + r lands at q * p2 of its patch in LDS, so that element ((c*pt + dt)*p1 + r)*p2 + col is in patch
// order and the bank rule above holds with q in the place of r.  An image is T = pt = 1.  No direct form: knob 13 only caps the span.
template <int VEC>
__global__ __launch_bounds__(256) void patch_nd_ln_fwd_kernel(
    const float* __restrict__ values, int64_t v_bstride, int64_t v_cstride, int64_t v_fstride, int64_t ldv, int gt, int gh, int npw,
    int C, int pt, int p1, int p2, int span, int n_span, int ps, int tw_log2, const float* __restrict__ gamma,
    const float* __restrict__ beta, float pad_value, float eps, float* __restrict__ xp, u16* __restrict__ xn, int64_t ld_bf16,
    int cols_pad, float* __restrict__ mean_out, float* __restrict__ rstd_out, uint8_t* __restrict__ padmask) {
  extern __shared__ __align__(16) float strip[];
  const int R = C * pt * p1, P = R * p2;
  int bid = blockIdx.x;
  const int sp = bid % n_span; bid /= n_span;
  const int hi = bid % gh; bid /= gh;
  const int ti = bid % gt;
  const int s = bid / gt;
  const int j0 = sp * span;
  const int cur = min(span, npw - j0);          // patches of this workgroup
  const int sw = cur * p2;                      // floats per strip row
  // element (c = 0, dt = 0, r = 0) of the span's first patch
  const float* src = values + (int64_t)s * v_bstride + (int64_t)ti * pt * v_fstride + (int64_t)hi * p1 * ldv + (int64_t)j0 * p2;
  // ---- stage: the R strip rows, coalesced, into patch order
  const int tx = threadIdx.x & ((1 << tw_log2) - 1), ty = threadIdx.x >> tw_log2, th = 256 >> tw_log2;
  for (int q = ty; q < R; q += th) {
    const int r = q % p1, cd = q / p1, dt = cd % pt, c = cd / pt;
    const float* srow = src + (int64_t)c * v_cstride + (int64_t)dt * v_fstride + (int64_t)r * ldv;
    float* drow = strip + q * p2;
    for (int cc = tx * VEC; cc < sw; cc += VEC << tw_log2) {
      const int j = cc / p2, col = cc - j * p2;          // (VEC = 4: p2 % 4 == 0, the four elements are of one run)
      if (VEC == 4) *reinterpret_cast<float4*>(drow + j * ps + col) = *reinterpret_cast<const float4*>(srow + cc);
      else drow[j * ps + col] = srow[cc];
    }
  }
  __syncthreads();
  // ---- normalise: one wavefront per patch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < cur; j += 4) {
    const int64_t row = (((int64_t)s * gt + ti) * gh + hi) * npw + j0 + j;
    const float* pr = strip + j * ps;
    patch_normalise<VEC>([&](int c) -> const float* { return pr + c; }, P, lane, row, gamma, beta, pad_value, eps, xp, xn, ld_bf16,
                         cols_pad, mean_out, rstd_out, padmask);
  }
}

extern "C" int mca_patch_ln_fwd(const float* values, int64_t v_bstride, int64_t ldv, int batch, int H, int W, int p1, int p2,
                                const float* gamma, const float* beta, float pad_value, float eps,
                                float* xp, uint16_t* xn_bf16, int64_t ld_bf16, int cols_pad,
                                float* mean, float* rstd, uint8_t* padmask, mca_stream_t stream) {
  if (!values || !gamma || !beta || !xn_bf16 || !mean || !rstd || !padmask) return MCA_E_BADARG;
  if (batch < 0 || H <= 0 || W <= 0 || p1 <= 0 || p2 <= 0 || H % p1 || W % p2) return MCA_E_BADARG;
  if ((int64_t)p1 * p2 > PATCH_MAX_P) return MCA_E_BADARG;
  const int P = p1 * p2;
  if (cols_pad < P || ld_bf16 < cols_pad || ldv < W) return MCA_E_BADARG;
  const int gh = H / p1, npw = W / p2;
  const int span = patch_span(P, npw), n_span = (npw + span - 1) / span, ps = patch_stride(P, p2);
  const int64_t nwg = (int64_t)batch * gh * n_span;
  if (nwg > 0x7fffffff || span * ps > PATCH_LDS_FLOATS) return MCA_E_BADARG;
  if (nwg == 0) return MCA_OK;
  const bool vec = p2 % 4 == 0 && ldv % 4 == 0 && v_bstride % 4 == 0 && ld_bf16 % 4 == 0 && (uintptr_t)values % 16 == 0 &&
                   (uintptr_t)xn_bf16 % 8 == 0 && (uintptr_t)xp % 16 == 0;
  const int groups = (span * p2 + (vec ? 3 : 0)) / (vec ? 4 : 1);          // column groups of a full strip row
  int tw_log2 = 0;
  while (tw_log2 < 8 && (1 << tw_log2) < groups) tw_log2++;
  const bool direct = mca_knobs[13] < 0;
  const size_t lds = direct ? 0 : (size_t)span * ps * sizeof(float);
#define PATCH_LAUNCH(VEC, DIRECT)                                                                                                  \
  hipLaunchKernelGGL((patch_ln_fwd_kernel<VEC, DIRECT>), dim3((unsigned)nwg), dim3(256), lds, as_stream(stream), values, v_bstride, \
                     ldv, gh, npw, p1, p2, span, n_span, ps, tw_log2, gamma, beta, pad_value, eps, xp, xn_bf16, ld_bf16, cols_pad,  \
                     mean, rstd, padmask)
  if (direct) { if (vec) PATCH_LAUNCH(4, true); else PATCH_LAUNCH(1, true); }
  else if (vec) PATCH_LAUNCH(4, false); else PATCH_LAUNCH(1, false);
#undef PATCH_LAUNCH
  return launch_status();
}

extern "C" int mca_patch_nd_ln_fwd(const float* values, int64_t v_bstride, int64_t v_cstride, int64_t v_fstride, int64_t ldv,
                                   int batch, int C, int T, int H, int W, int pt, int p1, int p2,
                                   const float* gamma, const float* beta, float pad_value, float eps,
                                   float* xp, uint16_t* xn_bf16, int64_t ld_bf16, int cols_pad,
                                   float* mean, float* rstd, uint8_t* padmask, mca_stream_t stream) {
  if (!values || !gamma || !beta || !xn_bf16 || !mean || !rstd || !padmask) return MCA_E_BADARG;
  if (batch < 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0 || pt <= 0 || p1 <= 0 || p2 <= 0 || T % pt || H % p1 || W % p2) return MCA_E_BADARG;
  if (C > PATCH_MAX_P || pt > PATCH_MAX_P || p1 > PATCH_MAX_P || p2 > PATCH_MAX_P) return MCA_E_BADARG;          // (the product below fits int64)
  if ((int64_t)C * pt * p1 * p2 > PATCH_MAX_P) return MCA_E_BADARG;
  const int P = C * pt * p1 * p2;
  if (cols_pad < P || ld_bf16 < cols_pad || ldv < W) return MCA_E_BADARG;
  // planes, frames and samples may be framed apart but not overlap: each stride covers the extent of what it steps over
  const int64_t plane = (int64_t)(H - 1) * ldv + W;
  if (T > 1 && v_fstride < plane) return MCA_E_BADARG;
  const int64_t clip = (int64_t)(T - 1) * v_fstride + plane;
  if (C > 1 && v_cstride < clip) return MCA_E_BADARG;
  if (batch > 1 && v_bstride < (int64_t)(C - 1) * v_cstride + clip) return MCA_E_BADARG;
  const int gt = T / pt, gh = H / p1, npw = W / p2;
  const int span = patch_nd_span(P, npw), n_span = (npw + span - 1) / span, ps = patch_stride(P, p2);
  const int64_t nwg = (int64_t)batch * gt * gh * n_span;
  if (nwg > 0x7fffffff || span * ps > PATCH_LDS_FLOATS) return MCA_E_BADARG;
  if (nwg == 0) return MCA_OK;
  const bool vec = p2 % 4 == 0 && ldv % 4 == 0 && v_fstride % 4 == 0 && v_cstride % 4 == 0 && v_bstride % 4 == 0 && ld_bf16 % 4 == 0 &&
                   (uintptr_t)values % 16 == 0 && (uintptr_t)xn_bf16 % 8 == 0 && (uintptr_t)xp % 16 == 0;
  const int groups = (span * p2 + (vec ? 3 : 0)) / (vec ? 4 : 1);          // column groups of a full strip row
  int tw_log2 = 0;
  while (tw_log2 < 8 && (1 << tw_log2) < groups) tw_log2++;
  const size_t lds = (size_t)span * ps * sizeof(float);
#define PATCH_ND_LAUNCH(VEC)                                                                                                        \
  hipLaunchKernelGGL((patch_nd_ln_fwd_kernel<VEC>), dim3((unsigned)nwg), dim3(256), lds, as_stream(stream), values, v_bstride,      \
                     v_cstride, v_fstride, ldv, gt, gh, npw, C, pt, p1, p2, span, n_span, ps, tw_log2, gamma, beta, pad_value, eps, \
                     xp, xn_bf16, ld_bf16, cols_pad, mean, rstd, padmask)
  if (vec) PATCH_ND_LAUNCH(4); else PATCH_ND_LAUNCH(1);
#undef PATCH_ND_LAUNCH
  return launch_status();
}
