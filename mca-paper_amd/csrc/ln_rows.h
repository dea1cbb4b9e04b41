// The row body of the trunk LayerNorm backward, two rows per wavefront (a and b) in the lane layout element (lane + 64 i) * 4,
// i < NI: shared by ln_bwd_trunk_kernel (elementwise.hip), which reads dy from memory, and by the full-row GEMM epilogue of
// gemm_nt_rows_kernel (gemm.hip), which takes dy from its own tile.  A row has to leave either with the same bits, so nothing
// here is left to the compiler: the functions are compiled with fp contraction OFF and say fmaf where a fused multiply-add is
// meant.  (Left to itself hipcc contracted differently from element to element of one row - s2 += g * xhat fused for the first
// float4 and not for the second, g - s1 folded into dy * gamma for four elements of row a only - and differently again in
// another kernel: last-bit differences in dx between two kernels running the same source text.)
#pragma once
#include "common.h"

// xhat overwrites x, g = dy * gamma overwrites dy; dg collects the lane's dgamma partials (row b only when `two`: without a
// second row b is a copy of a); s1 = mean(g), s2 = mean(g * xhat) of each row on return
template <int NI>
__device__ __forceinline__ void ln_bwd_rows_stats(float4 (&xa)[NI], float4 (&xb)[NI], float4 (&da)[NI], float4 (&db)[NI], const float4 (&gm)[NI],
                                                  float4 (&dg)[NI], float ma, float ra, float mb, float rb, bool two, float inv_cols,
                                                  float& s1a, float& s2a, float& s1b, float& s2b) {
#pragma clang fp contract(off)
  s1a = 0.f; s2a = 0.f; s1b = 0.f; s2b = 0.f;
#define LNB_ELEM(X, D, G, DG, M, R, S1, S2, LIVE)  { const float xh_ = ((X) - (M)) * (R); const float g_ = (D) * (G); if (LIVE) (DG) = __builtin_fmaf((D), xh_, (DG)); \
                                                    (S1) += g_; (S2) = __builtin_fmaf(g_, xh_, (S2)); (X) = xh_; (D) = g_; }
#pragma unroll
  for (int i = 0; i < NI; i++) {
    LNB_ELEM(xa[i].x, da[i].x, gm[i].x, dg[i].x, ma, ra, s1a, s2a, true)  LNB_ELEM(xa[i].y, da[i].y, gm[i].y, dg[i].y, ma, ra, s1a, s2a, true)
    LNB_ELEM(xa[i].z, da[i].z, gm[i].z, dg[i].z, ma, ra, s1a, s2a, true)  LNB_ELEM(xa[i].w, da[i].w, gm[i].w, dg[i].w, ma, ra, s1a, s2a, true)
    LNB_ELEM(xb[i].x, db[i].x, gm[i].x, dg[i].x, mb, rb, s1b, s2b, two)   LNB_ELEM(xb[i].y, db[i].y, gm[i].y, dg[i].y, mb, rb, s1b, s2b, two)
    LNB_ELEM(xb[i].z, db[i].z, gm[i].z, dg[i].z, mb, rb, s1b, s2b, two)   LNB_ELEM(xb[i].w, db[i].w, gm[i].w, dg[i].w, mb, rb, s1b, s2b, two)
  }
#undef LNB_ELEM
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1a += __shfl_xor(s1a, o, WAVE); s2a += __shfl_xor(s2a, o, WAVE); s1b += __shfl_xor(s1b, o, WAVE); s2b += __shfl_xor(s2b, o, WAVE);
  }
  s1a *= inv_cols; s2a *= inv_cols; s1b *= inv_cols; s2b *= inv_cols;
}

// dx of four elements, rstd * (g - s1 - xhat * s2): g and xhat as ln_bwd_rows_stats left dy and x
__device__ __forceinline__ float4 ln_bwd_row_dx(const float4& g, const float4& xh, float r, float s1, float s2) {
#pragma clang fp contract(off)
  float4 o;
  o.x = r * __builtin_fmaf(-xh.x, s2, g.x - s1); o.y = r * __builtin_fmaf(-xh.y, s2, g.y - s1);
  o.z = r * __builtin_fmaf(-xh.z, s2, g.z - s1); o.w = r * __builtin_fmaf(-xh.w, s2, g.w - s1);
  return o;
}
__device__ __forceinline__ uint2 ln_pack4bf(const float4& o) { uint2 pk; pk.x = pack2bf(o.x, o.y); pk.y = pack2bf(o.z, o.w); return pk; }
