// Attention readout (reference: model.py:87-103 - Attention.forward with return_attn=True hands back softmax(q·kᵀ) after the two
// masked_fill(-finfo.max)).  The (b,h,N,N) matrix is never written: per query row the kernel sums the probabilities by KEY GROUP
// (modality m = group m, fusion sub-block c = group M + c), and on request writes the probabilities of a window of rows.
//
// The probabilities come from the log-sum-exp the forward left behind: p_ij = exp2(q_i·k_j - lse_i) for an allowed, un-padded
// key, so no online maximum and no second pass are needed.  Tiling, tile lists, K staging and the orientation of the score
// product are the forward's (attention_fwd.hip): one workgroup per 128-row query tile of a (sample, head), 4 wavefronts x 32
// rows, S^T[key][q] = K · Q^T with v_mfma_f32_32x32x16_bf16, so that a LANE owns a query row and its 32 keys of a 64-key tile
// sit in its registers (key 32 kb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3) in register r of block kb).
//
// Group sums, fp32, fixed order, no atomics: the lower lane half of a row owns that row's G accumulators in LDS.  Key groups
// are long runs, so the sum is kept as a RUN: (group, partial sum) in registers, flushed into the LDS accumulator only when
// the group changes.  A 32-key block whose keys all share one group (almost all of them) is one 16-term register sum, one
// cross-half move and one add into the run; a mixed block (a structure boundary, the end of a sample's valid keys, the 8-key
// fusion sub-blocks) walks its keys in order.  Every step is the same on every launch: the result is bitwise repeatable.
//
// A row the forward marked uniform (lse = +inf: no allowed, un-padded key; the reference's softmax of a constant row) gets the
// host's uniform_mass (key count of the group / nk) and 1 / nk for every key, padded and blocked ones included.
#include "attention_common.h"

#define ACC_LD 33   // row stride of the group accumulators: 32 groups (31 = padded keys, never read back) + 1 (LDS banks)
#define MIXED 255u  // a 32-key block with more than one group

__global__ __launch_bounds__(256, 4) void attn_readout_kernel(mca_attn_readout_args a, float inv_nk) {
  __shared__ __attribute__((aligned(16))) u16 Ks[2 * AK * DH];          // K double-buffered: 16 KiB
  __shared__ __attribute__((aligned(16))) uint8_t kinfo[2][AK];
  __shared__ float acc[AQ * ACC_LD];                                    // per-row group sums: 16.5 KiB
  __shared__ uint8_t flags_s[MAX_KTILES];       // this sample's key-tile flags
  __shared__ uint8_t seen_s[MAX_KTILES];        // the tile is on this workgroup's live list (probs: the others are zero-filled)
  __shared__ uint32_t live_s[MAX_KTILES];
  __shared__ uint8_t uni_s[AQ];
  __shared__ int n_live_s;

  const auto [lin0, qt, h, b] = attn_wg_decode(a.q_order, 0);          // (no knob: always the XCD-aware order)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int arow = wave * 32 + l31;          // row inside the tile
  bool qvalid;
  const int qrow = attn_qrow(qt, arow, a.nq, qvalid);

  bf16x8 qf[4];
  attn_load_qf(qf, a.q + (int64_t)b * a.q_bstride + (int64_t)qrow * a.q_ld + h * DH, lh);
  const uint32_t qm = a.qmask[qrow];
  const float lse = a.lse[((int64_t)b * a.heads + h) * a.nq + qrow];
  const bool uniform = lse == INFINITY;

  const u16* kbase = a.k + (int64_t)b * a.kv_bstride + h * DH;
  const uint8_t* kinfo_g = a.keyinfo + (int64_t)b * a.nk_pad;
  {
    const uint8_t* flags_g = a.ktile_flags + (int64_t)b * a.n_ktiles;
    for (int i = tid; i < a.n_ktiles; i += 256) { flags_s[i] = flags_g[i]; seen_s[i] = 0; }
    for (int i = tid; i < AQ * ACC_LD; i += 256) acc[i] = 0.f;
    if (lh == 0) uni_s[arow] = uniform ? 1 : 0;
  }
  __syncthreads();

  // the rows of this tile inside the probs window
  const int w_lo = a.row0 > qt * AQ ? a.row0 : qt * AQ;
  int w_hi = a.row0 + a.n_rows;
  if (w_hi > (qt + 1) * AQ) w_hi = (qt + 1) * AQ;
  if (w_hi > a.nq) w_hi = a.nq;
  const bool do_probs = a.probs != nullptr && w_lo < w_hi;
  float* const pb = do_probs ? a.probs + ((int64_t)b * a.heads + h) * a.n_rows * (int64_t)a.nk : nullptr;
  const bool my_probs = do_probs && qvalid && qrow >= a.row0 && qrow < a.row0 + a.n_rows;
  float* const prow = my_probs ? pb + (int64_t)(qrow - a.row0) * a.nk : nullptr;

  // staging (the forward's register-staged form): 512 chunks of 16 B per K tile, 2 per thread
  int srow[2], sc[2];
  unsigned loff[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int id = tid + 256 * i; srow[i] = id >> 3; sc[i] = id & 7;
    loff[i] = (unsigned)(srow[i] * (int)a.kv_ld + sc[i] * 8);
  }
  const int last_kt = a.n_ktiles - 1;
  bf16x8 rk[2];
  uint32_t rinfo = 0;
  auto gload = [&](int kt) {
    if (tid < 16) rinfo = *reinterpret_cast<const uint32_t*>(kinfo_g + kt * AK + tid * 4);
    const u16* kb = kbase + (int64_t)kt * AK * a.kv_ld;
    if (kt != last_kt) {
#pragma unroll
      for (int i = 0; i < 2; i++) rk[i] = *reinterpret_cast<const bf16x8*>(kb + loff[i]);
    } else {          // rows past nk: re-read the last valid row (their keyinfo is 31: they add nothing)
#pragma unroll
      for (int i = 0; i < 2; i++) {
        int key = kt * AK + srow[i]; if (key > a.nk - 1) key = a.nk - 1;
        rk[i] = *reinterpret_cast<const bf16x8*>(kbase + (int64_t)key * a.kv_ld + sc[i] * 8);
      }
    }
  };
  auto swrite = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; i++) *reinterpret_cast<bf16x8*>(Ks + buf * AK * DH + k_off(srow[i], sc[i])) = rk[i];
    if (tid < 16) *reinterpret_cast<uint32_t*>(&kinfo[buf][tid * 4]) = rinfo;
  };

  // the tile list of this query tile, minus tiles whose keys are all padded in this sample (wavefront 0 compacts it).  Not
  // attn_compact_tiles: this one drops bit 31, bounds every entry and position, and marks the tiles it keeps in seen_s
  if (wave == 0) {
    const int lb = a.q_ptr[qt], le = a.q_ptr[qt + 1];
    int n = 0;
    for (int i0 = lb; i0 < le; i0 += 64) {
      const int i = i0 + lane;
      const uint32_t e = i < le ? (a.q_kt[i] & 0x7fffffffu) : 0u;
      const bool keep = i < le && e < (uint32_t)a.n_ktiles && flags_s[e] != 0;
      const unsigned long long m = __ballot(keep);
      const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
      if (keep && pos < MAX_KTILES) { live_s[pos] = e; seen_s[e] = 1; }
      n += __popcll(m);
    }
    if (lane == 0) n_live_s = n;
  }
  __syncthreads();
  const int it_end = n_live_s < MAX_KTILES ? n_live_s : MAX_KTILES;

  // probs of the key tiles this query tile never visits (not on the schedule, or every key padded): 0, or 1 / nk on a uniform row
  if (do_probs) {
    const int nr = w_hi - w_lo;
    for (int t = 0; t < a.n_ktiles; t++) {
      if (seen_s[t]) continue;
      for (int idx = tid; idx < nr * AK; idx += 256) {
        const int r = w_lo + (idx >> 6), key = t * AK + (idx & 63);
        if (key < a.nk) pb[(int64_t)(r - a.row0) * a.nk + key] = uni_s[r - qt * AQ] ? inv_nk : 0.f;
      }
    }
  }

  int it = 0, buf = 0;
  if (it < it_end) { gload((int)live_s[0]); swrite(0); }
  __syncthreads();

  // the running group sum of this lane's row (lower lane half only): flushed into acc when the group changes
  uint32_t cur_g = 31;
  float cur = 0.f;
  float* const arow_acc = acc + arow * ACC_LD;
  auto run_add = [&](uint32_t g, float v) {
    if (g != cur_g) { arow_acc[cur_g] += cur; cur = 0.f; cur_g = g; }
    cur += v;
  };

  while (it < it_end) {
    const int kt = (int)live_s[it];
    const int nit = it + 1;
    if (nit < it_end) gload((int)live_s[nit]);
    const u16* ks = Ks + buf * AK * DH;

    // the group of each 32-key block, if it has one: lane l looks at key l of the tile
    uint32_t bg[2];
    {
      const uint32_t mine = kinfo[buf][lane] & 31u;
      const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 0), g1 = (uint32_t)__builtin_amdgcn_readlane((int)mine, 32);
      const unsigned long long m = __ballot(mine == (lh ? g1 : g0));
      bg[0] = (uint32_t)m == 0xffffffffu ? g0 : MIXED;
      bg[1] = (uint32_t)(m >> 32) == 0xffffffffu ? g1 : MIXED;
    }
#pragma unroll
    for (int kb = 0; kb < 2; kb++) {
      // ---- S^T = K Q^T for 32 keys
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; r++) s[r] = 0.f;
#pragma unroll
      for (int st = 0; st < 4; st++) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + k_off(kb * 32 + l31, 2 * st + lh));
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[st], s, 0, 0, 0);
      }
      float p[16];
      if (bg[kb] != MIXED) {          // (wave-uniform) one group: one sum
        const bool ok = (qm >> bg[kb]) & 1u;          // padded keys are group 31: no query has that bit
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) { p[r] = ok ? __builtin_amdgcn_exp2f(s[r] - lse) : 0.f; t += p[r]; }
        t += __shfl_xor(t, 32, WAVE);
        if (lh == 0) run_add(bg[kb], t);
      } else {                        // a boundary inside the block: key by key, in key order
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const uint32_t own4 = *reinterpret_cast<const uint32_t*>(&kinfo[buf][kb * 32 + 8 * g + 4 * lh]);
          const uint32_t oth4 = *reinterpret_cast<const uint32_t*>(&kinfo[buf][kb * 32 + 8 * g + 4 * (lh ^ 1)]);
          float po[4];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const uint32_t grp = (own4 >> (8 * e)) & 0xffu;
            p[4 * g + e] = ((qm >> (grp & 31u)) & 1u) ? __builtin_amdgcn_exp2f(s[4 * g + e] - lse) : 0.f;
            po[e] = __shfl_xor(p[4 * g + e], 32, WAVE);
          }
          if (lh == 0) {          // keys 8g .. 8g+3 are this lane's, 8g+4 .. 8g+7 the upper half's
#pragma unroll
            for (int e = 0; e < 4; e++) run_add((own4 >> (8 * e)) & 31u, p[4 * g + e]);
#pragma unroll
            for (int e = 0; e < 4; e++) run_add((oth4 >> (8 * e)) & 31u, po[e]);
          }
        }
      }
      if (my_probs) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int key = kt * AK + kb * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
          if (key < a.nk) prow[key] = uniform ? inv_nk : p[r];
        }
      }
    }

    if (nit < it_end) swrite(buf ^ 1);
    __syncthreads();
    buf ^= 1;
    it = nit;
  }
  if (lh == 0) arow_acc[cur_g] += cur;
  __syncthreads();

  // ---- mass: the wavefront's 32 rows x G are contiguous
  const int G = a.n_groups;
  const int row_base = qt * AQ + wave * 32;
  int nrows = a.nq - row_base; if (nrows > 32) nrows = 32;
  if (nrows > 0) {
    float* mp = a.mass + (((int64_t)b * a.heads + h) * a.nq + row_base) * G;
    for (int idx = lane; idx < nrows * G; idx += 64) {
      const int r = idx / G, g = idx - r * G;
      mp[idx] = uni_s[wave * 32 + r] ? a.uniform_mass[g] : acc[(wave * 32 + r) * ACC_LD + g];
    }
  }
}

extern "C" int mca_attn_readout(const mca_attn_readout_args* a, mca_stream_t stream) {
  if (!a || !a->q || !a->k || !a->lse || !a->qmask || !a->keyinfo || !a->ktile_flags || !a->q_ptr || !a->q_kt || !a->q_order ||
      !a->uniform_mass || !a->mass)
    return MCA_E_BADARG;
  if (a->batch <= 0 || a->heads <= 0 || a->nq <= 0 || a->nk <= 0) return MCA_E_BADARG;
  if (a->n_groups < 1 || a->n_groups > 31) return MCA_E_BADARG;
  if (a->probs && (a->row0 < 0 || a->n_rows <= 0 || a->row0 >= a->nq || a->n_rows > a->nq - a->row0)) return MCA_E_BADARG;
  if (a->n_qtiles != (a->nq + AQ - 1) / AQ || a->n_ktiles != (a->nk + AK - 1) / AK) return MCA_E_BADARG;
  if (a->nk_pad < a->n_ktiles * AK || a->nk_pad % 4) return MCA_E_BADARG;
  if (a->q_ld % 8 || a->kv_ld % 8 || a->q_bstride % 8 || a->kv_bstride % 8) return MCA_E_ALIGN;
  if ((uintptr_t)a->q % 16 || (uintptr_t)a->k % 16 || (uintptr_t)a->keyinfo % 4) return MCA_E_ALIGN;
  if (a->heads > 65535 || a->batch > 65535 || a->n_ktiles > MAX_KTILES || (int64_t)a->kv_ld * 64 >= (1ll << 31)) return MCA_E_UNSUPPORTED;
  if (!(a->flags & MCA_ATTN_Q_PRESCALED)) return MCA_E_UNSUPPORTED;
  hipLaunchKernelGGL(attn_readout_kernel, dim3(a->n_qtiles, a->heads, a->batch), dim3(256), 0, as_stream(stream), *a,
                     1.0f / (float)a->nk);
  return launch_status();
}
