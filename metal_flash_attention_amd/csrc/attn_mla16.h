// attn_mla16.h -- multi-head latent attention (MLA) decode over a compressed KV cache on the 16-bit matrix cores of gfx950
// (include/mfa_mla.h): every query head reads the ONE cache row of a key, Dk = 576 columns as its key and the first
// Dv = 512 as its value.  Not an instantiation of attn_decode16.h: a wave's O^T accumulator there is D x 32 and register-bound at
// D = 256, so here the four waves of a workgroup SHARE every 32-key step and divide its columns instead.
//
//   * one workgroup (4 waves) serves one group of 32 packed query rows (p = head x R + row) of one sequence, and one piece of its keys.
//   * wave w owns the latent columns [128 w, 128 w + 128) and the rotary columns [512 + 16 w, 512 + 16 w + 16): 144 of the 576.  It
//     loads exactly that slice of the step's 32 key rows STRAIGHT to registers as the A operand (a lane = a key row, nine 16-byte loads,
//     36 VGPRs): a column of the cache is fetched once per workgroup and serves both products.
//   * partial S^T over the slice: nine v_mfma_f32_32x32x16 against the wave's Q slice (36 VGPRs, loaded once).  The four partials meet
//     in LDS (a 16 KiB exchange buffer, two of them used in turn: a wave may write the next step's partial while a slower one still
//     reads this step's, so ONE workgroup barrier per step is enough -- a buffer is rewritten two steps later, behind the barrier of the
//     step between).  Every wave reads the four partials and adds them in the SAME order, ((w0 + w1) + w2) + w3: the waves hold
//     bit-identical scores and run the same softmax, so (m, l) and P need no further exchange.
//   * the wave then multiplies P by ITS OWN 128 latent columns: the eight latent fragments it holds go to a wave-private LDS image
//     [4][32 keys][32 d] (8 KiB) and come back as V^T through ds_read_b64_tr_b16, as decode does, into a 128 x 32 O^T slice (64 VGPRs).
//     The rotary fragment never enters the second product.
//   * the next step's loads are issued as soon as this step's registers are consumed (after the image writes, before the exchange).
//   * what may hold poison is never loaded: key rows at or past the piece's end come in as zeros, a masked score is REPLACED (p = 0
//     exactly) and the running maximum only ever sees visible keys (attn_cache_step.h) -- a piece without a visible key keeps
//     m = -FLT_MAX, l = 0.
//   * keys are addressed in groups of 16 (a step starts on a multiple of 32 and a page holds at least 16 keys): two wave-uniform
//     block-table reads per step, none per lane.
//   * the end: every wave holds the row's (m, l) and its own 128 columns of O^T; it normalises and stores them straight from registers
//     (a lane's four consecutive d are one 8- or 16-byte store); wave 0 stores L.  SPLIT: piece s of sequence b takes
//     decode_piece_range(len_b, pieces, s) -- the function the host exports -- and publishes un-normalised O and (m, l) in FP32 (wsO
//     [pieces][B H R][Dv], wsML [pieces][B H R][2]); attn_mla16_combine merges them.
#pragma once
#include "attn_cache_step.h"
#include "attn_decode16.h"

namespace mfa {

constexpr int MLA_DK = 576, MLA_DV = 512;
constexpr int MLA_ROWS = 32;                     // packed rows of a workgroup (MFA_MLA_PACKED_ROWS)
constexpr int MLA_WAVES = 4, MLA_STEP = 32;
constexpr int MLA_LATENT = MLA_DV / MLA_WAVES;   // 128 latent columns of a wave
constexpr int MLA_ROPE = (MLA_DK - MLA_DV) / MLA_WAVES;   // 16 rotary columns of a wave
constexpr int MLA_NKS = (MLA_LATENT + MLA_ROPE) / 16;     // 9 matrix steps of the wave's slice
constexpr int MLA_NDB = MLA_LATENT / 32;                  // 4 d blocks of the wave's O^T slice
constexpr int MLA_IMAGE = MLA_STEP * MLA_LATENT * 2;      // bytes of a wave's V image
constexpr int MLA_XBUF = MLA_WAVES * 16 * 64 * 4;         // bytes of one exchange buffer: a partial S^T per wave
constexpr int MLA_LDS = MLA_WAVES * MLA_IMAGE + 2 * MLA_XBUF;   // 64 KiB

struct MlaArgs {
  const char *q, *kv;
  char *o;
  float *l;                       // null: not stored
  const uint32_t *lengths;
  const int32_t *table;           // paged launches
  int64_t tableStride;
  int64_t ldq, hsq, bsq;          // elements
  int64_t ldk, bsk, psk;
  int64_t ldo, hso, bso;
  int64_t lhs, lbs;
  uint32_t R, H, M, groups, batches, column;   // M = H R packed rows, in `groups` groups of 32
  uint32_t paged, pageShift;      // pageSize = 1 << pageShift
  uint32_t causal, outF32;
  uint32_t pieces;
  float scale2;                   // fl(scale x log2 e)
  float *wsO, *wsML;
  const float *kvScale;           // the e4m3 kernels only (attn_mla8.h), one entry; null: 1.0.  Last, so that no other field moves
};

template <typename T, bool SPLIT>
__device__ __forceinline__ void mla_decode_body(const MlaArgs &a) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t piece = SPLIT ? blockIdx.x % a.pieces : 0u;
  const uint32_t gb = SPLIT ? blockIdx.x / a.pieces : blockIdx.x;
  const uint32_t group = gb % a.groups, batch = gb / a.groups;
  const uint32_t R = a.R, M = a.M;
  const uint32_t len = min(a.lengths[batch], a.column);
  uint32_t begin = 0, end = len;
  if constexpr (SPLIT) decode_piece_range(len, a.pieces, piece, &begin, &end);

  // ---- the lane's packed query row; rows at or past M repeat the last one and are not stored
  const uint32_t p = group * MLA_ROWS + (uint32_t)q;
  const uint32_t pc = min(p, M - 1);
  const uint32_t head = pc / R, qrow = pc % R;
  // the wave's slice: fragment t < 8 is the latent columns 128 w + 16 t .. + 15, fragment 8 the rotary columns 512 + 16 w .. + 15;
  // a lane holds the 8 columns from 8 hi of each
  const int col0 = MLA_LATENT * wave + 8 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  v8 qf[MLA_NKS];
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t)
      qf[t] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (t < 8 ? col0 + 16 * t : colR) * 2));
  }
  // keys this row sees (causal: c <= row + max(len - R, 0); always c < len, and inside this piece c < end)
  const VisibleKeys<false, false> keys(end, qrow + (len > R ? len - R : 0u) + 1u, a.causal, 0u, 0u);

  // ---- addresses of a step's two 16-key groups (wave-uniform; element offsets from a.kv)
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  auto group_offsets = [&](uint32_t key0, int64_t (&ko)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t key = key0 + 16u * u;
      if (a.paged) {
        // (entries past the piece's last key are never read)
        const int64_t page = key < end ? (int64_t)a.table[(int64_t)batch * a.tableStride + (key >> a.pageShift)] : 0;
        ko[u] = page * a.psk + (int64_t)(key & pageMask) * a.ldk;
      } else {
        ko[u] = (int64_t)batch * a.bsk + (int64_t)key * a.ldk;
      }
    }
  };

  // lane = key row q of the step, its slice of the row as the A operand
  u32x4 kreg[MLA_NKS];
  auto issue_loads = [&](uint32_t key0) {
    int64_t ko[2];
    group_offsets(key0, ko);
    const bool kvalid = key0 + (uint32_t)q < end;
    const char *kp = a.kv + ((q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk) * 2;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + (t < 8 ? col0 + 16 * t : colR) * 2);
      kreg[t] = z;
    }
  };

  f32x16 o[MLA_NDB];
  float m = STEP_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d]
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  uint32_t key0 = begin, buf = 0;
  if (key0 < end) issue_loads(key0);
  while (key0 < end) {   // (the same trips for every wave: the barrier below is met by all)
    // ---- the wave's partial S^T = K Q^T over its 144 columns: s[r] = key key0 + crow(r, hi), packed query row q
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t) s = F::mfma(__builtin_bit_cast(v8, kreg[t]), qf[t], s);
    // ---- the latent fragments to the wave's image (its previous reads were issued before these writes: one wave, in order):
    // fragment t is the columns 16 (t & 1) + 8 hi .. + 7 of d block t >> 1
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<u32x4 *>(Vs + ((t >> 1) * MLA_STEP + q) * 64 + (t & 1) * 32 + hi * 16) = kreg[t];
    // ---- the registers are free: the next step's loads fly during the rest of this one
    const uint32_t cur = key0;
    key0 += MLA_STEP;
    if (key0 < end) issue_loads(key0);

    // ---- the four partials meet: [buffer][wave][4][64 lanes] float4
    float4 *xb = reinterpret_cast<float4 *>(xchg + buf * MLA_XBUF);
#pragma unroll
    for (int g = 0; g < 4; ++g) xb[(wave * 4 + g) * 64 + lane] = make_float4(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 x0 = xb[(0 * 4 + g) * 64 + lane], x1 = xb[(1 * 4 + g) * 64 + lane];
      const float4 x2 = xb[(2 * 4 + g) * 64 + lane], x3 = xb[(3 * 4 + g) * 64 + lane];
      s[4 * g] = ((x0.x + x1.x) + x2.x) + x3.x;
      s[4 * g + 1] = ((x0.y + x1.y) + x2.y) + x3.y;
      s[4 * g + 2] = ((x0.z + x1.z) + x2.z) + x3.z;
      s[4 * g + 3] = ((x0.w + x1.w) + x2.w) + x3.w;
    }
    buf ^= 1u;

    // ---- online softmax over the visible keys only: the same arithmetic on the same values in every wave
    rescale_row(score_max<true>(s, keys, cur, hi, a.scale2), m, l, o);
    v8 pf[2];
    l += score_exp<T, true>(s, keys, cur, hi, m, pf);

    // ---- O^T += V^T P^T over the wave's 128 latent columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < MLA_NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[u], o[db]);
  }

  // ---- every wave holds the row's (m, l) and its own columns of O^T: no merge.  o[db][4 g + i] is d = 128 w + 32 db + 8 g + 4 hi + i
  const float l_tot = l + __shfl_xor(l, 32);
  if (p >= M) return;   // (no barrier follows)
  float mult = 1.0f;
  if constexpr (!SPLIT) mult = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // a sequence of length 0: O = 0
  const size_t slab = ((size_t)piece * a.batches + batch) * M + p;
  const int64_t at0 = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)qrow * a.ldo;
#pragma unroll
  for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = MLA_LATENT * wave + 32 * db + 8 * g + 4 * hi;
      const float4 x = make_float4(o[db][4 * g] * mult, o[db][4 * g + 1] * mult, o[db][4 * g + 2] * mult, o[db][4 * g + 3] * mult);
      if constexpr (SPLIT) *reinterpret_cast<float4 *>(a.wsO + slab * MLA_DV + d) = x;
      else store_o4<T>(a.o, at0 + d, a.outF32, x);
    }
  if (wave == 0 && hi == 0) {
    if constexpr (SPLIT) *reinterpret_cast<float2 *>(a.wsML + slab * 2) = make_float2(m, l_tot);
    else if (a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + qrow] = row_lse(m, l_tot);
  }
}

// Merge the pieces at Dv = 512 (decode's combine body assumes D / 4 <= 64 column lanes per row).  One wave per query row: lane s holds
// (m_s, l_s) of piece s (pieces <= 64); for O a lane owns the float4 columns lane and lane + 64 and walks the pieces in order.  A
// piece without keys has l = 0: its weight is 0 and its slab is not read.
template <typename T>
__device__ __forceinline__ void mla_combine_body(const MlaArgs &a) {
  const int lane = threadIdx.x & 63;
  const uint32_t S = a.pieces;
  const uint64_t rows = (uint64_t)a.batches * a.M;
  const uint64_t rowid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rowid >= rows) return;
  const uint32_t pr = (uint32_t)(rowid % a.M), batch = (uint32_t)(rowid / a.M);
  const uint32_t head = pr / a.R, row = pr % a.R;
  float ms = STEP_MINUS_HUGE, ls = 0.f;
  if ((uint32_t)lane < S) {
    const float2 ml = *reinterpret_cast<const float2 *>(a.wsML + ((uint64_t)lane * rows + rowid) * 2);
    ms = ml.x; ls = ml.y;
  }
  if (!(ls > 0.f)) ms = STEP_MINUS_HUGE;   // (an empty piece never sets the maximum)
  float mstar = ms;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mstar = fmaxf(mstar, __shfl_xor(mstar, off, 64));
  const float w = ((uint32_t)lane < S && ls > 0.f) ? fast_exp2(ms - mstar) : 0.f;
  float lstar = w * ls;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) lstar += __shfl_xor(lstar, off, 64);
  float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  for (uint32_t s_ = 0; s_ < S; ++s_) {
    const float ws = __shfl(w, (int)s_, 64);
    if (ws > 0.f) {   // (wave-uniform)
      const float *src = a.wsO + ((uint64_t)s_ * rows + rowid) * MLA_DV;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float4 x = *reinterpret_cast<const float4 *>(src + (lane + 64 * j) * 4);
        acc[j].x += ws * x.x; acc[j].y += ws * x.y; acc[j].z += ws * x.z; acc[j].w += ws * x.w;
      }
    }
  }
  const float inv = lstar > 0.f ? 1.0f / lstar : 0.f;
  const int64_t at = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)row * a.ldo;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    acc[j].x *= inv; acc[j].y *= inv; acc[j].z *= inv; acc[j].w *= inv;
    store_o4<T>(a.o, at + (lane + 64 * j) * 4, a.outF32, acc[j]);
  }
  if (lane == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + row] = row_lse(mstar, lstar);
}

} // namespace mfa
