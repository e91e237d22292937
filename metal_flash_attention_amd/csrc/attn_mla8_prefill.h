// attn_mla8_prefill.h -- multi-head latent attention PREFILL over an E4M3 latent cache (include/mfa_mla_prefill_fp8.h):
// attn_mla16_prefill.h's workgroup with attn_mla8.h's read.  A sibling of mla_prefill_body, as mla8_decode_body is a sibling of
// mla_decode_body, not a flag on it: the 16-bit prefill kernels stay the instructions they were.  From attn_mla16_prefill.h, unchanged:
// the row-major packing p = row x H + head, one workgroup (4 waves) a block of 64 packed rows as TWO tiles of 32, wave w owning the
// latent columns [128 w, + 128) and the rotary columns [512 + 16 w, + 16), mla_prefill_step_range and mla_prefill_split_piece_range,
// the exchange [tile][wave][4][64] float4 in two buffers behind ONE barrier a step, the order ((w0 + w1) + w2) + w3,
// rescale_row_uniform, score_max / score_exp in their masked and unmasked forms, vt_mfma over the one image for both tiles, the
// epilogue's layout, 96 KiB of LDS.  What changes is attn_mla8.h's list:
//   * loads.  A lane (= a key row of the step) loads its wave's slice as BYTES: four 16-byte loads at 128 w + 32 t + 16 hi and one
//     8-byte load at 512 + 16 w + 8 hi -- 18 registers where the 16-bit kernel holds 36.  One step of loads in flight, issued as soon
//     as the step's conversions are done.
//   * conversion, ONCE a step for BOTH tiles.  cvt8_e4m3<T> (kv_e4m3.h: exact) turns a 16-byte load into two A fragments; they feed
//     the matrix instructions of tile 0 and of tile 1 and go to the wave's V image, and only then is the next load converted: eight
//     registers of converted values live at a time, never the whole slice (72).  The conversion and the image write are paid once for
//     64 packed rows where the decode kernel pays them for 32.
//   * contraction order.  Q fragment 2 t + j is the columns 128 w + 32 t + 16 hi + 8 j .. + 7, the order of the K bytes; the rotary
//     fragment keeps its order.
//   * V image in TRUE d order: a lane's 16 values of load t are d 32 t + 16 hi .. + 15 of d block t.
//   * scale.  One uniform load of kvScale[0].  The score scale is fl(scale2 x kvScale); the unsplit epilogue multiplies by
//     fl(fl(1 / l) x kvScale); a piece publishes fl(o x kvScale) un-normalised, so mla_prefill_combine_body serves unchanged.
//   * poison is the bytes 0x7f / 0xff: key rows at or past n come in as zero bytes (+0.0), block-table entries past the last page are
//     not read, nothing in a last page's tail or in a page no table names is loaded.
// For every packed row the arithmetic is mla8_decode_body<T, false>'s, bit for bit: the same nine-instruction chain in the same
// order, the same order of the partials, the same step header, the same normalisation and stores.  A step past a row's frontier changes
// no bit of the row, so a row's result depends neither on its block nor on how a prompt is cut into chunks.
#pragma once
#include "attn_mla16_prefill.h"
#include "attn_mla8.h"

namespace mfa {

// MlaPrefillArgs as it is (mla_prefill_combine_body reads `a`), and the cache's scale behind it
struct Mla8PrefillArgs {
  MlaPrefillArgs a;
  const float *kvScale;   // device, one entry; null: 1.0
};

template <typename T, bool SPLIT>
__device__ __forceinline__ void mla8_prefill_body(const Mla8PrefillArgs &args) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NL = MLA_LATENT / 32;   // 4 16-byte loads of the wave's latent slice, one d block each
  const MlaPrefillArgs &a = args.a;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t piece = SPLIT ? blockIdx.x % a.pieces : 0u;   // (fastest: a block's pieces are neighbours)
  const uint32_t bb = SPLIT ? blockIdx.x / a.pieces : blockIdx.x;
  const uint32_t block = bb % a.blocks, batch = bb / a.blocks;
  const uint32_t H = a.H;
  const uint32_t n = min(a.lengths[batch], a.column);
  const uint32_t qn = a.qlengths ? min(a.qlengths[batch], a.R) : a.R;
  const uint32_t p0 = block * (uint32_t)MLAP_ROWS;
  if (p0 / H >= qn) return;   // (the whole workgroup, ahead of every barrier)
  uint32_t firstMasked, stepEnd;
  mla_prefill_step_range(n, qn, p0, H, a.causal, &firstMasked, &stepEnd);
  const uint32_t live = qn * H;   // packed rows of the sequence
  uint32_t stepBegin = 0;
  if constexpr (SPLIT) {
    mla_prefill_split_piece_range(stepEnd, a.pieces, piece, &stepBegin, &stepEnd);
    if (stepBegin >= stepEnd) {   // a piece without a step: (m, l) = (-FLT_MAX, 0) for the live rows, no O (the whole workgroup, ahead
      const uint32_t p = p0 + (uint32_t)tid;   // of every barrier)
      if (tid < MLAP_ROWS && p < live)
        *reinterpret_cast<float2 *>(a.wsML + (((size_t)piece * a.batches + batch) * ((size_t)a.R * H) + p) * 2) = make_float2(STEP_MINUS_HUGE, 0.f);
      return;
    }
  }
  const float kvs = args.kvScale ? args.kvScale[0] : 1.0f;
  const float kscale = a.scale2 * kvs;   // the cache's scale rides on the softmax scale

  // ---- the lane's packed query row of each tile; rows at or past `live` repeat the last live one and are not stored.  The wave's
  // slice in the order of the K bytes: fragment 2 t + j < 8 is the latent columns 128 w + 32 t + 16 hi + 8 j .. + 7, fragment 8 the
  // rotary columns 512 + 16 w + 8 hi .. + 7
  const int col0 = MLA_LATENT * wave + 16 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
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
      qf[t][k] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (k < 8 ? col0 + 32 * (k >> 1) + 8 * (k & 1) : colR) * 2));
  }
  // keys a row sees (causal: c <= row + max(n - qn, 0); always c < n)
  const uint32_t off = n > qn ? n - qn : 0u;
  const VisibleKeys<false, false> keys[MLAP_TILES] = {VisibleKeys<false, false>(n, qrow[0] + off + 1u, a.causal, 0u, 0u),
                                                      VisibleKeys<false, false>(n, qrow[1] + off + 1u, a.causal, 0u, 0u)};

  // ---- addresses of a step's two 16-key groups (wave-uniform; byte offsets from a.kv)
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

  // lane = key row q of the step, its slice of the row as bytes: the A operand of both tiles once converted
  u32x4 klat[NL];
  u32x2 krope;
  auto issue_loads = [&](uint32_t key0) {
    int64_t ko[2];
    group_offsets(key0, ko);
    const bool kvalid = key0 + (uint32_t)q < n;
    const char *kp = a.kv + (q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk;
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + col0 + 32 * t);
      klat[t] = z;
    }
    u32x2 z = {0u, 0u};
    if (kvalid) z = *reinterpret_cast<const u32x2 *>(kp + colR);
    krope = z;
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

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d], 16-bit values, read by both tiles
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  const uint32_t keyEnd = stepEnd * (uint32_t)MLA_STEP, unmaskedEnd = firstMasked * (uint32_t)MLA_STEP;
  uint32_t key0 = stepBegin * (uint32_t)MLA_STEP, buf = 0;
  if (key0 < keyEnd) issue_loads(key0);
  while (key0 < keyEnd) {   // (the same trips for every wave: the barrier below is met by all)
    // ---- the wave's partial S^T = K Q^T over its 144 columns, one per tile: s[t][r] = key key0 + crow(r, hi), packed row q of tile
    // t.  A load is converted once, feeds both tiles' two matrix instructions and goes to the wave's image (its previous reads were
    // issued before these writes: one wave, in order) before the next load is converted
    f32x16 s[MLAP_TILES];
#pragma unroll
    for (int t = 0; t < MLAP_TILES; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
    for (int c = 0; c < NL; ++c) {
      const u32x4 k0 = cvt8_e4m3<T>(klat[c][0], klat[c][1]), k1 = cvt8_e4m3<T>(klat[c][2], klat[c][3]);
#pragma unroll
      for (int t = 0; t < MLAP_TILES; ++t) {
        s[t] = F::mfma(__builtin_bit_cast(v8, k0), qf[t][2 * c], s[t]);
        s[t] = F::mfma(__builtin_bit_cast(v8, k1), qf[t][2 * c + 1], s[t]);
      }
      char *dst = Vs + (c * MLA_STEP + q) * 64 + hi * 32;
      *reinterpret_cast<u32x4 *>(dst) = k0;
      *reinterpret_cast<u32x4 *>(dst + 16) = k1;
    }
    {
      const u32x4 kr = cvt8_e4m3<T>(krope[0], krope[1]);
#pragma unroll
      for (int t = 0; t < MLAP_TILES; ++t) s[t] = F::mfma(__builtin_bit_cast(v8, kr), qf[t][8], s[t]);
    }
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
        __builtin_amdgcn_sched_barrier(0);   // (four reads in flight at a time, as attn_mla16_prefill.h)
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
      mx[t] = unmasked ? score_max<false>(s[t], keys[t], cur, hi, kscale) : score_max<true>(s[t], keys[t], cur, hi, kscale);
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
  // (no barrier follows).  The cache's scale multiplies what leaves the workgroup.  SPLIT: un-normalised, to the piece's slab
#pragma unroll
  for (int t = 0; t < MLAP_TILES; ++t) {
    const float l_tot = l[t] + __shfl_xor(l[t], 32);
    const uint32_t p = p0 + (uint32_t)(MLA_ROWS * t + q);
    if (p >= live) continue;
    float mult = kvs;
    if constexpr (!SPLIT) mult = l_tot > 0.f ? (1.0f / l_tot) * kvs : 0.f;   // a row without a visible key: O = 0
    const size_t slab = SPLIT ? ((size_t)piece * a.batches + batch) * ((size_t)a.R * H) + p : 0;
    const int64_t at0 = (int64_t)batch * a.bso + (int64_t)head[t] * a.hso + (int64_t)qrow[t] * a.ldo;
#pragma unroll
    for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = MLA_LATENT * wave + 32 * db + 8 * g + 4 * hi;
        const float4 x = make_float4(o[t][db][4 * g] * mult, o[t][db][4 * g + 1] * mult, o[t][db][4 * g + 2] * mult, o[t][db][4 * g + 3] * mult);
        if constexpr (SPLIT) *reinterpret_cast<float4 *>(a.wsO + slab * MLA_DV + d) = x;
        else store_o4<T>(a.o, at0 + d, a.outF32, x);
      }
    if (wave == 0 && hi == 0) {
      if constexpr (SPLIT) *reinterpret_cast<float2 *>(a.wsML + slab * 2) = make_float2(m[t], l_tot);
      else if (a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head[t] * a.lhs + qrow[t]] = row_lse(m[t], l_tot);
    }
  }
}

} // namespace mfa
