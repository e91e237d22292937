// attn_mla16_prefill.h -- multi-head latent attention PREFILL over the compressed KV cache (include/mfa_mla_prefill.h):
// a block of new query rows per sequence, of any length, on the pieces of attn_mla16.h and the step of attn_cache_step.h.
//
//   * packing is ROW-major, p = row x H + head: the 64 packed rows of a workgroup are the heads of as few rows as can be, so that they
//     share a causal frontier as nearly as they can.  One workgroup (4 waves) serves one block of 64 packed rows of one sequence as TWO
//     tiles of 32 (tile t: the rows p0 + 32 t .. + 31; lane & 31 is the row of BOTH tiles).
//   * the division of a step is attn_mla16.h's: wave w owns the latent columns [128 w, 128 w + 128) and the rotary columns
//     [512 + 16 w, + 16), loads that slice of the step's 32 key rows straight to registers (36 VGPRs) ONCE, and that one load serves
//     both tiles and both products: nine matrix instructions a tile against the tile's Q slice (2 x 36 VGPRs), the eight latent
//     fragments to the wave's V image (8 KiB, shared by the tiles), and P V into the tile's own 128 x 32 O^T slice (2 x 64 registers).
//   * the partials of both tiles meet in LDS behind ONE barrier a step (an exchange buffer is [tile][wave][4][64] float4 = 32 KiB, two
//     used in turn as in attn_mla16.h); every wave adds them in the same order, ((w0 + w1) + w2) + w3, and runs the same softmax.
//   * mla_prefill_step_range -- one function, device and host (mfa_attention_mla_prefill_step_range) -- gives the block its steps:
//     [0, firstMasked) run score_max<false> / score_exp<.., false>, [firstMasked, end) with the per-element mask, steps at or past end
//     are never loaded.  A step past a row's own frontier is fully masked for that row: p = 0, the maximum untouched, +0 added -- no
//     bit of the row changes, so a row's result does not depend on the block it falls in.
//   * for every packed row the arithmetic is mla_decode_body<T, false>'s, bit for bit: the same nine-instruction chains, the same order
//     of the partials, the same step header, the same normalisation and stores.
//   * what may hold poison is never loaded: key rows at or past n come in as zeros, block-table entries past the last page are not
//     read, lanes at or past the last live packed row repeat it and store nothing, rows at or past qn are never read.
//   * LDS: 4 x 8 KiB images + 2 x 32 KiB exchange buffers = 96 KiB; one workgroup a compute unit, up to 512 registers a lane.
#pragma once
#include "attn_mla16.h"

namespace mfa {

constexpr int MLAP_TILES = 2;
constexpr int MLAP_ROWS = MLAP_TILES * MLA_ROWS;                 // packed rows of a workgroup (MFA_MLA_PREFILL_PACKED_ROWS)
constexpr int MLAP_XBUF = MLAP_TILES * MLA_XBUF;                 // bytes of one exchange buffer
constexpr int MLAP_LDS = MLA_WAVES * MLA_IMAGE + 2 * MLAP_XBUF;  // 96 KiB

struct MlaPrefillArgs {
  const char *q, *kv;
  char *o;
  float *l;                       // null: not stored
  const uint32_t *lengths;
  const uint32_t *qlengths;       // null: every sequence has R rows
  const int32_t *table;           // paged launches
  int64_t tableStride;
  int64_t ldq, hsq, bsq;          // elements
  int64_t ldk, bsk, psk;
  int64_t ldo, hso, bso;
  int64_t lhs, lbs;
  uint32_t R, H, blocks, batches, column;   // R = the rows' capacity; `blocks` blocks of 64 packed rows a sequence
  uint32_t paged, pageShift;      // pageSize = 1 << pageShift
  uint32_t causal, outF32;
  float scale2;                   // fl(scale x log2 e)
};

// The 32-key steps of the block of the 64 packed rows from p0 (p = row x H + head) of a sequence of n keys and qn rows: row r sees the
// keys c < lim(r) = min(n, r + max(n - qn, 0) + 1) (not causal: n), which grows with r.  *end = ceil(lim(last live row) / 32): no live
// row of the block sees a key of a step at or past it.  *firstMasked = floor(lim(first row) / 32): every key of a step below it is
// visible to every live row.  Device and host run this one body.
__host__ __device__ __forceinline__ void mla_prefill_step_range(uint32_t n, uint32_t qn, uint32_t p0, uint32_t H, uint32_t causal,
                                                                uint32_t *firstMasked, uint32_t *end) {
  const uint64_t r0 = p0 / H;
  if (r0 >= qn || n == 0) {
    *firstMasked = *end = 0;
    return;
  }
  uint64_t lo = n, hi = n;
  if (causal) {
    const uint64_t off = n > qn ? (uint64_t)n - qn : 0;
    uint64_t last = ((uint64_t)p0 + MLAP_ROWS - 1) / H;   // the block's last row, live or not
    if (last > (uint64_t)qn - 1) last = (uint64_t)qn - 1;
    lo = r0 + off + 1;
    hi = last + off + 1;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
  }
  const uint64_t e = (hi + MLA_STEP - 1) / MLA_STEP;
  uint64_t f = lo / MLA_STEP;
  if (f > e) f = e;
  *firstMasked = (uint32_t)f;
  *end = (uint32_t)e;
}

// rescale_row (attn_cache_step.h) behind a WAVE-uniform test: a lane whose maximum does not rise multiplies by 1.0f, which changes no
// bit, so the row's arithmetic is rescale_row's.  (With 128 accumulators a lane the per-lane branch made hipcc spill them.)
template <int NDB> __device__ __forceinline__ void rescale_row_uniform(float mx, float &m, float &l, f32x16 (&o)[NDB]) {
  const bool up = mx > m;
  if (__builtin_amdgcn_ballot_w64(up) != 0) {
    const float corr = up ? fast_exp2(m - mx) : 1.0f;
    m = up ? mx : m;
    l *= corr;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= corr;
  }
}

template <typename T>
__device__ __forceinline__ void mla_prefill_body(const MlaPrefillArgs &a) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t block = blockIdx.x % a.blocks, batch = blockIdx.x / a.blocks;
  const uint32_t H = a.H;
  const uint32_t n = min(a.lengths[batch], a.column);
  const uint32_t qn = a.qlengths ? min(a.qlengths[batch], a.R) : a.R;
  const uint32_t p0 = block * (uint32_t)MLAP_ROWS;
  if (p0 / H >= qn) return;   // (the whole workgroup, ahead of every barrier)
  uint32_t firstMasked, stepEnd;
  mla_prefill_step_range(n, qn, p0, H, a.causal, &firstMasked, &stepEnd);
  const uint32_t live = qn * H;   // packed rows of the sequence

  // ---- the lane's packed query row of each tile; rows at or past `live` repeat the last live one and are not stored
  const int col0 = MLA_LATENT * wave + 8 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  uint32_t head[MLAP_TILES], qrow[MLAP_TILES];
  v8 qf[MLAP_TILES][MLA_NKS];
#pragma unroll
  for (int t = 0; t < MLAP_TILES; ++t) {
    const uint32_t pc = min(p0 + (uint32_t)(MLA_ROWS * t + q), live - 1);
    head[t] = pc % H;
    qrow[t] = pc / H;
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head[t] * a.hsq + (int64_t)qrow[t] * a.ldq) * 2;
#pragma unroll
    for (int k = 0; k < MLA_NKS; ++k)
      qf[t][k] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (k < 8 ? col0 + 16 * k : colR) * 2));
  }
  // keys a row sees (causal: c <= row + max(n - qn, 0); always c < n)
  const uint32_t off = n > qn ? n - qn : 0u;
  const VisibleKeys<false, false> keys[MLAP_TILES] = {VisibleKeys<false, false>(n, qrow[0] + off + 1u, a.causal, 0u, 0u),
                                                      VisibleKeys<false, false>(n, qrow[1] + off + 1u, a.causal, 0u, 0u)};

  // ---- addresses of a step's two 16-key groups (wave-uniform; element offsets from a.kv)
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  auto group_offsets = [&](uint32_t key0, int64_t (&ko)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t key = key0 + 16u * u;
      if (a.paged) {
        // (entries past the sequence's last key are never read)
        const int64_t page = key < n ? (int64_t)a.table[(int64_t)batch * a.tableStride + (key >> a.pageShift)] : 0;
        ko[u] = page * a.psk + (int64_t)(key & pageMask) * a.ldk;
      } else {
        ko[u] = (int64_t)batch * a.bsk + (int64_t)key * a.ldk;
      }
    }
  };

  // lane = key row q of the step, its slice of the row as the A operand of both tiles
  u32x4 kreg[MLA_NKS];
  auto issue_loads = [&](uint32_t key0) {
    int64_t ko[2];
    group_offsets(key0, ko);
    const bool kvalid = key0 + (uint32_t)q < n;
    const char *kp = a.kv + ((q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk) * 2;
#pragma unroll
    for (int k = 0; k < MLA_NKS; ++k) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + (k < 8 ? col0 + 16 * k : colR) * 2);
      kreg[k] = z;
    }
  };

  f32x16 o[MLAP_TILES][MLA_NDB];
  float m[MLAP_TILES], l[MLAP_TILES];
#pragma unroll
  for (int t = 0; t < MLAP_TILES; ++t) {
    m[t] = STEP_MINUS_HUGE;
    l[t] = 0.f;
#pragma unroll
    for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][db][r] = 0.f;
  }

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d], read by both tiles
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  const uint32_t keyEnd = stepEnd * (uint32_t)MLA_STEP, unmaskedEnd = firstMasked * (uint32_t)MLA_STEP;
  uint32_t key0 = 0, buf = 0;
  if (key0 < keyEnd) issue_loads(key0);
  while (key0 < keyEnd) {   // (the same trips for every wave: the barrier below is met by all)
    // ---- the wave's partial S^T = K Q^T over its 144 columns, one per tile: s[t][r] = key key0 + crow(r, hi), packed row q of tile t
    f32x16 s[MLAP_TILES];
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
      for (int k = 0; k < MLA_NKS; ++k) s[t] = F::mfma(__builtin_bit_cast(v8, kreg[k]), qf[t][k], s[t]);
    }
    // ---- the latent fragments to the wave's image (its previous reads were issued before these writes: one wave, in order)
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<u32x4 *>(Vs + ((k >> 1) * MLA_STEP + q) * 64 + (k & 1) * 32 + hi * 16) = kreg[k];
    // ---- the registers are free: the next step's loads fly during the rest of this one
    const uint32_t cur = key0;
    key0 += MLA_STEP;
    if (key0 < keyEnd) issue_loads(key0);

    // ---- the partials meet: [buffer][tile][wave][4][64 lanes] float4
    float4 *xb = reinterpret_cast<float4 *>(xchg + buf * MLAP_XBUF);
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        xb[((t * MLA_WAVES + wave) * 4 + g) * 64 + lane] = make_float4(s[t][4 * g], s[t][4 * g + 1], s[t][4 * g + 2], s[t][4 * g + 3]);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        __builtin_amdgcn_sched_barrier(0);   // (four reads in flight at a time: the form that was measured; sixteen a tile are untried)
        const float4 *xt = xb + (t * MLA_WAVES * 4 + g) * 64 + lane;
        const float4 x0 = xt[0 * 4 * 64], x1 = xt[1 * 4 * 64], x2 = xt[2 * 4 * 64], x3 = xt[3 * 4 * 64];
        s[t][4 * g] = ((x0.x + x1.x) + x2.x) + x3.x;
        s[t][4 * g + 1] = ((x0.y + x1.y) + x2.y) + x3.y;
        s[t][4 * g + 2] = ((x0.z + x1.z) + x2.z) + x3.z;
        s[t][4 * g + 3] = ((x0.w + x1.w) + x2.w) + x3.w;
      }
    }
    buf ^= 1u;

    // ---- online softmax, the step header of attn_cache_step.h per tile: the same arithmetic on the same values in every wave
    v8 pf[MLAP_TILES][2];
    float mx[MLAP_TILES];
    const bool unmasked = cur < unmaskedEnd;   // (workgroup-uniform) every key of the step is visible to every row of the block
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t)
      mx[t] = unmasked ? score_max<false>(s[t], keys[t], cur, hi, a.scale2) : score_max<true>(s[t], keys[t], cur, hi, a.scale2);
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t) rescale_row_uniform(mx[t], m[t], l[t], o[t]);
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t)
      l[t] += unmasked ? score_exp<T, false>(s[t], keys[t], cur, hi, m[t], pf[t]) : score_exp<T, true>(s[t], keys[t], cur, hi, m[t], pf[t]);

    // ---- O^T += V^T P^T over the wave's 128 latent columns, both tiles from the one image
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int db = 0; db < MLA_NDB; ++db) o[t][db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[t][u], o[t][db]);
  }

  // ---- every wave holds the rows' (m, l) and its own columns of O^T: no merge.  o[t][db][4 g + i] is d = 128 w + 32 db + 8 g + 4 hi + i
  // (no barrier follows)
#pragma unroll
  for (int t = 0; t < MLAP_TILES; ++t) {
    const float l_tot = l[t] + __shfl_xor(l[t], 32);
    if (p0 + (uint32_t)(MLA_ROWS * t + q) >= live) continue;
    const float mult = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // a row without a visible key: O = 0
    const int64_t at0 = (int64_t)batch * a.bso + (int64_t)head[t] * a.hso + (int64_t)qrow[t] * a.ldo;
#pragma unroll
    for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = MLA_LATENT * wave + 32 * db + 8 * g + 4 * hi;
        store_o4<T>(a.o, at0 + d, a.outF32,
                    make_float4(o[t][db][4 * g] * mult, o[t][db][4 * g + 1] * mult, o[t][db][4 * g + 2] * mult, o[t][db][4 * g + 3] * mult));
      }
    if (wave == 0 && hi == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head[t] * a.lhs + qrow[t]] = row_lse(m[t], l_tot);
  }
}

} // namespace mfa
