// attn_mla8.h -- multi-head latent attention decode over an E4M3 latent cache (include/mfa_mla_cache.h): the body of
// attn_mla16.h with the cache row read as 576 BYTES.  A sibling of mla_decode_body, not a parameter of it: the 16-bit kernels stay
// the instructions they were.  The partition is attn_mla16.h's -- four waves share each 32-key step, wave w owns the latent columns
// [128 w, 128 w + 128) and the rotary columns [512 + 16 w, + 16), partial S^T meets in the double-buffered LDS exchange with one
// barrier a step, every wave adds the partials in the same order and runs the same softmax, and P multiplies the wave's own 128
// latent columns from its private V image through ds_read_b64_tr_b16 -- and so are MlaArgs, decode_piece_range, the workspace slabs
// and the combine kernel.  What changes:
//   * loads.  A lane (= a key row) loads its wave's slice as bytes: four 16-byte loads at 128 w + 32 t + 16 hi and one 8-byte load at
//     512 + 16 w + 8 hi -- 18 VGPRs where the 16-bit kernel holds 36.
//   * conversion.  cvt8_e4m3<T> (kv_e4m3.h: exact) turns a 16-byte load into two A fragments at their matrix instructions; the
//     16-bit v_mfma_f32_32x32x16 is kept (the launch is bound by bytes).
//   * contraction order.  Fragment (t, j) of a lane holds the columns 128 w + 32 t + 16 hi + 8 j .. + 7: the latent contraction is
//     permuted against the 16-bit kernel's, and the Q fragments are loaded in the same permuted order (the FP8 side of
//     attn_decode16.h).  The rotary fragment keeps its order.
//   * V image.  The converted latent values go to the image in TRUE d order: a lane's 16 values of load t are d 32 t + 16 hi .. + 15
//     of d block t.  vt_mfma and the O^T layout are untouched.
//   * scale.  One uniform load of kvScale[0] at the start.  It multiplies scale2 -- fl(fl(scale log2 e) x kvScale), the softmax pays
//     nothing -- and the final `mult`; a piece multiplies the un-normalised O it publishes, so the combine kernel, linear in O,
//     needs no change.
//   * poison here is the bytes 0x7f / 0xff: key rows at or past the piece's end come in as zero bytes (+0.0); nothing past a length,
//     in a last page's tail or in a page no table names is loaded.
// One step of loads in flight, as attn_mla16.h.  -DMFA_MLA8_FLIGHT=2 builds the measured alternative, two register sets taken in turn
// (216 registers for 183): inside the spread of one step where the launch is bound by bytes, so not the product.
#pragma once
#include "attn_mla16.h"
#include "kv_e4m3.h"

namespace mfa {

#ifndef MFA_MLA8_FLIGHT
#define MFA_MLA8_FLIGHT 1
#endif
constexpr int MLA8_FLIGHT = MFA_MLA8_FLIGHT;   // steps of loads in flight: FLIGHT register sets of 18, taken in turn

template <typename T, bool SPLIT>
__device__ __forceinline__ void mla8_decode_body(const MlaArgs &a) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NL = MLA_LATENT / 32;   // 4 16-byte loads of the wave's latent slice, one d block each

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
  const float kvs = a.kvScale ? a.kvScale[0] : 1.0f;
  const float kscale = a.scale2 * kvs;   // the cache's scale rides on the softmax scale

  // ---- the lane's packed query row; rows at or past M repeat the last one and are not stored
  const uint32_t p = group * MLA_ROWS + (uint32_t)q;
  const uint32_t pc = min(p, M - 1);
  const uint32_t head = pc / R, qrow = pc % R;
  // the wave's slice in the order of the K bytes: fragment 2 t + j < 8 is the latent columns 128 w + 32 t + 16 hi + 8 j .. + 7,
  // fragment 8 the rotary columns 512 + 16 w + 8 hi .. + 7
  const int col0 = MLA_LATENT * wave + 16 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  v8 qf[MLA_NKS];
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int s = 0; s < MLA_NKS; ++s)
      qf[s] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (s < 8 ? col0 + 32 * (s >> 1) + 8 * (s & 1) : colR) * 2));
  }
  // keys this row sees (causal: c <= row + max(len - R, 0); always c < len, and inside this piece c < end)
  const VisibleKeys<false, false> keys(end, qrow + (len > R ? len - R : 0u) + 1u, a.causal, 0u, 0u);

  // ---- addresses of a step's two 16-key groups (wave-uniform; byte offsets from a.kv)
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

  // lane = key row q of the step, its slice of the row as bytes
  struct KSlice {
    u32x4 latent[NL];
    u32x2 rope;
  };
  KSlice held[MLA8_FLIGHT];
  auto issue_loads = [&](KSlice &k, uint32_t key0) {
    int64_t ko[2];
    group_offsets(key0, ko);
    const bool kvalid = key0 + (uint32_t)q < end;
    const char *kp = a.kv + (q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk;
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + col0 + 32 * t);
      k.latent[t] = z;
    }
    u32x2 z = {0u, 0u};
    if (kvalid) z = *reinterpret_cast<const u32x2 *>(kp + colR);
    k.rope = z;
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

  uint32_t buf = 0;
  // one 32-key step from key `cur` out of the register set k, which then takes the loads of the step at `next`
  auto step = [&](KSlice &k, uint32_t cur, uint32_t next) {
    // ---- the wave's partial S^T = K Q^T over its 144 columns, a load converted at its two matrix instructions; the converted latent
    // values go to the wave's image on the way (its previous reads were issued before these writes: one wave, in order): the 16
    // values of load t are the columns 16 hi .. + 15 of d block t
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
    // ---- the registers are free: the loads of the set's next step fly during the rest of this one
    if (next < end) issue_loads(k, next);

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
    rescale_row(score_max<true>(s, keys, cur, hi, kscale), m, l, o);
    v8 pf[2];
    l += score_exp<T, true>(s, keys, cur, hi, m, pf);

    // ---- O^T += V^T P^T over the wave's 128 latent columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < MLA_NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[u], o[db]);
  };

  uint32_t key0 = begin;
#pragma unroll
  for (int f = 0; f < MLA8_FLIGHT; ++f)
    if (key0 + f * MLA_STEP < end) issue_loads(held[f], key0 + f * MLA_STEP);
  while (key0 < end) {   // (the same trips for every wave: the barrier of a step is met by all)
#pragma unroll
    for (int f = 0; f < MLA8_FLIGHT; ++f)
      if (key0 < end) {
        step(held[f], key0, key0 + MLA8_FLIGHT * MLA_STEP);
        key0 += MLA_STEP;
      }
  }

  // ---- every wave holds the row's (m, l) and its own columns of O^T: no merge.  o[db][4 g + i] is d = 128 w + 32 db + 8 g + 4 hi + i.
  // The cache's scale multiplies what leaves the workgroup.
  const float l_tot = l + __shfl_xor(l, 32);
  if (p >= M) return;   // (no barrier follows)
  float mult = kvs;
  if constexpr (!SPLIT) mult = l_tot > 0.f ? (1.0f / l_tot) * kvs : 0.f;   // a sequence of length 0: O = 0
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

} // namespace mfa
