// attn_mla8_prefill_sparse.h -- SPARSE multi-head latent attention PREFILL over an E4M3 latent cache
// (include/mfa_mla_prefill_sparse_fp8.h): the rule of attn_mla16_prefill_sparse.h over the cache format of attn_mla8.h.
// A body of its own, mla8_prefill_sparse_body<T>: a sibling of mla_prefill_sparse_body and of mla8_sparse_decode_body, not a flag on
// either -- both stay the instructions they were measured with.
//   From attn_mla16_prefill_sparse.h, ONE tile: the packing (a workgroup of four waves serves 32 HEADS of ONE (sequence, row); grid
//     batches x rows x groups, group fastest; a workgroup whose row is at or past qn = min(queryLengths[b], rows) returns ahead of every
//     barrier, having read neither Q nor its list; lanes of heads at or past H repeat the last head and store nothing), the list walk
//     (lane q of step i owns slot 32 i + q; valid iff c < lim, one unsigned compare, lim = causal ? min(n, qrow + max(n - qn, 0) + 1) : n
//     with n = min(cacheLengths[b], column); a hole's table entry is never read, nothing past slot topk - 1 is read; the step's mask is
//     the low word of the ballot; the rows of step i + 1 are issued inside step i, the page of step i + 2 and the positions of step
//     i + 3 behind them) and the step (the partials of the four waves behind ONE barrier in two exchange buffers, added as
//     ((w0 + w1) + w2) + w3; rescale_row_uniform; score_max<true> / score_exp<T, true> over the mask; vt_mfma over the wave's image).
//     The two-tile variant is not carried: it lost in 16-bit for registers and LDS, and two tiles' O^T (128 registers) plus two Q
//     slices (72) still leave one wave a SIMD here.
//   From attn_mla8.h / attn_mla8_sparse.h: the row of a lane is read as BYTES -- four 16-byte loads at 128 w + 32 t + 16 hi, one 8-byte
//     load at 512 + 16 w + 8 hi: 18 registers where the 16-bit body holds 36 --, cvt8_e4m3<T> converts a 16-byte load at its two matrix
//     instructions, the Q fragments are in the permuted order of the K bytes, the converted latent values go to the wave's V image in
//     true d order on the way, and there is one uniform load of kvScale[0] (null: 1.0): the score scale is fl(scale2 x kvScale), the
//     epilogue multiplies by fl(fl(1 / l) x kvScale).  Row addresses are BYTE offsets: the 16-bit body's `* 2` has no counterpart.
//   A hole's row is zero bytes (+0.0) and is never loaded; a step of 32 holes has mask 0 and leaves (m, l, O) bit for bit.  A row
//   without a visible slot gets O = 0 and L = -FLT_MAX.
// For every live row the arithmetic is mla8_sparse_decode_body<T, false>'s, bit for bit (a lane whose maximum does not rise multiplies
// by 1.0f): 32 full rows equal the unsplit sparse e4m3 decode launch, the identity list equals the unsplit e4m3 prefill launch.
// LDS: 4 x 8 KiB images + 2 x 16 KiB exchange buffers = 64 KiB; __launch_bounds__(256, 2), two workgroups a compute unit.
// One step of rows in flight: 208 vector registers, 84 scalar, no scratch, no spills (read off the built gfx950 code object, both types;
// the 16-bit body holds 225).
// -DMFA_MLA8PX_FLIGHT=2 builds the alternative of attn_mla8_sparse.h: two register sets of 18 taken in turn, with the positions and the
// pages fetched one step further ahead.  It is not the product.
#pragma once
#include "attn_mla16_prefill_sparse.h"
#include "attn_mla8.h"

namespace mfa {

#ifndef MFA_MLA8PX_FLIGHT
#define MFA_MLA8PX_FLIGHT 1
#endif
constexpr int MLA8PX_FLIGHT = MFA_MLA8PX_FLIGHT;   // steps of rows in flight: FLIGHT register sets of 18, taken in turn
constexpr int MLA8PX_LDS = mlapx_lds<1>();

// MlaPrefillSparseArgs as it is, and the cache's scale behind it
struct Mla8PrefillSparseArgs {
  MlaPrefillSparseArgs s;
  const float *kvScale;   // device, one entry; null: 1.0
};

template <typename T>
__device__ __forceinline__ void mla8_prefill_sparse_body(const Mla8PrefillSparseArgs &args) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NL = MLA_LATENT / 32;   // 4 16-byte loads of the wave's latent slice, one d block each
  constexpr uint32_t FL = (uint32_t)MLA8PX_FLIGHT;
  const MlaPrefillSparseArgs &sa = args.s;
  const MlaPrefillArgs &a = sa.a;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t group = blockIdx.x % a.blocks, br = blockIdx.x / a.blocks;
  const uint32_t R = a.R, H = a.H;
  const uint32_t qrow = br % R, batch = br / R;
  const uint32_t qn = a.qlengths ? min(a.qlengths[batch], R) : R;
  if (qrow >= qn) return;   // (the whole workgroup, ahead of every barrier: neither Q nor the list of such a row is read)
  const uint32_t n = min(a.lengths[batch], a.column);
  // positions this row sees: c < lim (an entry below 0 is a huge unsigned number)
  const uint32_t lim = a.causal ? min(n, qrow + (n > qn ? n - qn : 0u) + 1u) : n;
  const uint32_t end = sa.topk;
  const float kvs = args.kvScale ? args.kvScale[0] : 1.0f;
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
  auto slot_position = [&](uint32_t slot0) -> uint32_t {   // (slots at or past topk are holes and are not read)
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
  KSlice held[MLA8PX_FLIGHT];
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

  // ---- the pipeline's start (topk >= 1): rows of the first FLIGHT steps; position and page of the step behind them, position of the
  // one after
  uint32_t key0 = 0, buf = 0;
  uint32_t cn, cn2;   // positions of the steps FLIGHT and FLIGHT + 1 ahead of the current one
  int32_t pagen;      // page of cn
  {
    uint32_t c0[MLA8PX_FLIGHT];
    int32_t page0[MLA8PX_FLIGHT];
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f) c0[f] = slot_position(f * MLA_STEP);
    cn = slot_position(FL * MLA_STEP);
    cn2 = slot_position((FL + 1) * MLA_STEP);
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f) page0[f] = position_page(c0[f]);
    pagen = position_page(cn);
#pragma unroll
    for (uint32_t f = 0; f < FL; ++f)
      if (f * MLA_STEP < end) issue_loads(held[f], c0[f], page0[f]);
  }

  // one 32-slot step from slot `cur` out of the register set k, which then takes the rows of the step FLIGHT further on
  auto step = [&](KSlice &k, uint32_t cur) {
    const ListedKeys keys{k.bits};   // one mask for the 32 heads: the heads of a row share its list
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
    rescale_row_uniform(score_max<true>(s, keys, 0u, hi, kscale), m, l, o);
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
    for (int f = 0; f < MLA8PX_FLIGHT; ++f)
      if (key0 < end) {
        step(held[f], key0);
        key0 += MLA_STEP;
      }
  }

  // ---- the end is the sparse decode body's, with the lane's head and the workgroup's row; the cache's scale multiplies what leaves
  const float l_tot = l + __shfl_xor(l, 32);
  if (hp >= H) return;   // (no barrier follows)
  const float mult = l_tot > 0.f ? (1.0f / l_tot) * kvs : 0.f;   // a row without a visible slot: O = 0
  const int64_t at0 = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)qrow * a.ldo;
#pragma unroll
  for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = MLA_LATENT * wave + 32 * db + 8 * g + 4 * hi;
      const float4 x = make_float4(o[db][4 * g] * mult, o[db][4 * g + 1] * mult, o[db][4 * g + 2] * mult, o[db][4 * g + 3] * mult);
      store_o4<T>(a.o, at0 + d, a.outF32, x);
    }
  if (wave == 0 && hi == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + qrow] = row_lse(m, l_tot);
}

} // namespace mfa
