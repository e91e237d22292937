// attn_mla8_sparse.h -- sparse MLA decode over an E4M3 latent cache (include/mfa_mla_sparse_fp8.h): the rule of
// attn_mla16_sparse.h over the cache format of attn_mla8.h.  A sibling of mla_sparse_decode_body and of mla8_decode_body, not a
// parameter of either: both stay the instructions they were.  MlaSparseArgs is unchanged (its MlaArgs carries kvScale).
//   From attn_mla16_sparse.h: the packing (32 HEADS of one (sequence, row) per workgroup; grid batches x rows x groups x pieces, pieces
//     fastest, then the group), pieces of SLOTS, the key of a lane (slot begin + 32 i + q, 0xFFFFFFFF at or past the piece's end, valid
//     iff c < lim: one unsigned comparison; paged: one table read per lane, a hole's entry is never read), the step's mask from the low
//     word of the ballot (ListedKeys), the prefetch of the table read and of the index read, and the end (head = 32 group + q, slab row
//     head x rows + row).
//   From attn_mla8.h: the row of a lane is read as BYTES -- four 16-byte loads at 128 w + 32 t + 16 hi, one 8-byte load at
//     512 + 16 w + 8 hi --, cvt8_e4m3<T> at the matrix instructions, the Q fragments in the same permuted order, the converted values
//     to the V image in true d order, and one uniform load of kvScale[0] folded into scale2 and into the final `mult` (a piece
//     multiplies the un-normalised O it publishes).  The contraction order, the order ((w0 + w1) + w2) + w3 of the partials and the
//     scale arithmetic are that header's: over the identity list, unsplit, this body gives mla8_decode_body's bits in O and L.
//   Row addresses are in BYTES: the 16-bit sparse body's `ko * 2` has no counterpart here.
//   A hole's row comes in as zero bytes (+0.0) and is never loaded; a step of 32 holes has mask 0 and leaves (m, l, O) bit for bit.
// One step of rows in flight (208 registers).  -DMFA_MLA8X_FLIGHT=2 builds the measured alternative: two register sets of 18 taken in
// turn, with the positions and the pages fetched one step further ahead (230 registers, still two workgroups a compute unit, no
// scratch).  It is 1.08 and 1.01 of one step's time on the rows the bytes bound and 0.97 - 0.99 where a launch is a chain of latencies
// (DESIGN.md 4.26): not the product.
#pragma once
#include "attn_mla16_sparse.h"
#include "attn_mla8.h"

namespace mfa {

#ifndef MFA_MLA8X_FLIGHT
#define MFA_MLA8X_FLIGHT 1
#endif
constexpr int MLA8X_FLIGHT = MFA_MLA8X_FLIGHT;   // steps of rows in flight: FLIGHT register sets of 18, taken in turn

template <typename T, bool SPLIT>
__device__ __forceinline__ void mla8_sparse_decode_body(const MlaSparseArgs &sa) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NL = MLA_LATENT / 32;   // 4 16-byte loads of the wave's latent slice, one d block each
  constexpr uint32_t FL = (uint32_t)MLA8X_FLIGHT;
  const MlaArgs &a = sa.a;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t piece = SPLIT ? blockIdx.x % a.pieces : 0u;
  const uint32_t gb = SPLIT ? blockIdx.x / a.pieces : blockIdx.x;
  const uint32_t group = gb % a.groups, br = gb / a.groups;
  const uint32_t R = a.R, H = a.H;
  const uint32_t qrow = br % R, batch = br / R;
  const uint32_t len = min(a.lengths[batch], a.column);
  // positions this row sees: c < lim (an entry below 0 is a huge unsigned number)
  const uint32_t lim = a.causal ? min(len, qrow + (len > R ? len - R : 0u) + 1u) : len;
  uint32_t begin = 0, end = sa.topk;
  if constexpr (SPLIT) decode_piece_range(sa.topk, a.pieces, piece, &begin, &end);
  const float kvs = a.kvScale ? a.kvScale[0] : 1.0f;
  const float kscale = a.scale2 * kvs;   // the cache's scale rides on the softmax scale

  // ---- the lane's head; heads at or past H repeat the last one and are not stored.  The wave's slice in the order of the K bytes
  // (attn_mla8.h): fragment 2 t + j < 8 is the latent columns 128 w + 32 t + 16 hi + 8 j .. + 7, fragment 8 the rotary columns
  const uint32_t hp = group * MLA_ROWS + (uint32_t)q;
  const uint32_t head = min(hp, H - 1);
  const int col0 = MLA_LATENT * wave + 16 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  v8 qf[MLA_NKS];
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int s = 0; s < MLA_NKS; ++s)
      qf[s] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (s < 8 ? col0 + 32 * (s >> 1) + 8 * (s & 1) : colR) * 2));
  }

  // ---- the list of this (sequence, row): slot -> position, position -> page
  const int32_t *list = sa.indices + (int64_t)batch * sa.ibs + (int64_t)qrow * sa.irs;
  const int32_t *table = a.table + (int64_t)batch * a.tableStride;
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  auto slot_position = [&](uint32_t slot0) -> uint32_t {   // (slots at or past the piece's end are holes and are not read)
    const uint32_t slot = slot0 + (uint32_t)q;
    return slot < end ? (uint32_t)list[slot] : 0xFFFFFFFFu;
  };
  auto position_page = [&](uint32_t c) -> int32_t {        // (the table entry of a hole is never read)
    return a.paged && c < lim ? table[c >> a.pageShift] : 0;
  };

  // lane = the key row of slot q of the step, its slice of the row as bytes; `bits` is the step's mask
  struct KSlice {
    u32x4 latent[NL];
    u32x2 rope;
    uint32_t bits;
  };
  KSlice held[MLA8X_FLIGHT];
  auto issue_loads = [&](KSlice &k, uint32_t c, int32_t page) {
    const bool kvalid = c < lim;
    // a BYTE offset: an element of an e4m3 cache is a byte
    const int64_t ko = a.paged ? (int64_t)page * a.psk + (int64_t)(c & pageMask) * a.ldk : (int64_t)batch * a.bsk + (int64_t)c * a.ldk;
    const char *kp = a.kv + ko;
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + col0 + 32 * t);
      k.latent[t] = z;
    }
    u32x2 z = {0u, 0u};
    if (kvalid) z = *reinterpret_cast<const u32x2 *>(kp + colR);
    k.rope = z;
    k.bits = (uint32_t)__ballot(kvalid);   // lanes 0 .. 31 are the step's slots
  };

  f32x16 o[MLA_NDB];
  float m = STEP_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d], 16-bit values
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  // ---- the pipeline's start: rows of the first FLIGHT steps; position and page of the step behind them, position of the one after
  uint32_t key0 = begin, buf = 0;
  uint32_t cn = 0xFFFFFFFFu, cn2 = 0xFFFFFFFFu;   // positions of the steps FLIGHT and FLIGHT + 1 ahead of the current one
  int32_t pagen = 0;                              // page of cn
  if (key0 < end) {
    uint32_t c0[MLA8X_FLIGHT];
    int32_t page0[MLA8X_FLIGHT];
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f) c0[f] = slot_position(key0 + f * MLA_STEP);
    cn = slot_position(key0 + FL * MLA_STEP);
    cn2 = slot_position(key0 + (FL + 1) * MLA_STEP);
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f) page0[f] = position_page(c0[f]);
    pagen = position_page(cn);
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f)
      if (key0 + f * MLA_STEP < end) issue_loads(held[f], c0[f], page0[f]);
  }

  // one 32-slot step from slot `cur` out of the register set k, which then takes the rows of the step FLIGHT further on
  auto step = [&](KSlice &k, uint32_t cur) {
    const ListedKeys keys{k.bits};
    // ---- the wave's partial S^T = K Q^T over its 144 columns, a load converted at its two matrix instructions; the converted latent
    // values go to the wave's image on the way (attn_mla8.h): the 16 values of load t are the columns 16 hi .. + 15 of d block t
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const u32x4 k0 = cvt8_e4m3<T>(k.latent[t][0], k.latent[t][1]), k1 = cvt8_e4m3<T>(k.latent[t][2], k.latent[t][3]);
      s = F::mfma(__builtin_bit_cast(v8, k0), qf[2 * t], s);
      s = F::mfma(__builtin_bit_cast(v8, k1), qf[2 * t + 1], s);
      char *dst = Vs + (t * MLA_STEP + q) * 64 + hi * 32;
      *reinterpret_cast<u32x4 *>(dst) = k0;
      *reinterpret_cast<u32x4 *>(dst + 16) = k1;
    }
    s = F::mfma(__builtin_bit_cast(v8, cvt8_e4m3<T>(k.rope[0], k.rope[1])), qf[8], s);
    // ---- the registers are free: the rows of the set's next step fly during the rest of this one, behind them the page of the step
    // after it and the positions of the step after that
    if (cur + FL * MLA_STEP < end) {
      issue_loads(k, cn, pagen);
      cn = cn2;
      pagen = position_page(cn);
      cn2 = slot_position(cur + (FL + 2) * MLA_STEP);
    }

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

    // ---- online softmax over the step's valid slots only: the same arithmetic on the same values in every wave
    rescale_row(score_max<true>(s, keys, 0u, hi, kscale), m, l, o);
    v8 pf[2];
    l += score_exp<T, true>(s, keys, 0u, hi, m, pf);

    // ---- O^T += V^T P^T over the wave's 128 latent columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < MLA_NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[u], o[db]);
  };

  while (key0 < end) {   // (the same trips for every wave: the barrier of a step is met by all)
#pragma unroll
    for (int f = 0; f < MLA8X_FLIGHT; ++f)
      if (key0 < end) {
        step(held[f], key0);
        key0 += MLA_STEP;
      }
  }

  // ---- the end is attn_mla16_sparse.h's, with the lane's head and the workgroup's row; the cache's scale multiplies what leaves
  const float l_tot = l + __shfl_xor(l, 32);
  if (hp >= H) return;   // (no barrier follows)
  float mult = kvs;
  if constexpr (!SPLIT) mult = l_tot > 0.f ? (1.0f / l_tot) * kvs : 0.f;   // a row without a visible slot: O = 0
  const size_t slab = ((size_t)piece * a.batches + batch) * a.M + (size_t)head * R + qrow;
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

} // namespace mfa
