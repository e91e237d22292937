// attn_cache_step.h -- what the kernels over a KV cache share (attn_decode16.h, attn_prefill16.h): which
// keys a query row sees, the online-softmax step over 32 keys with its O^T += V^T P^T, the sink-logit fold, and how O and L leave
// the kernel.  Both kernels hold a packed query row per lane (the fragment maps of dev/attn_fwd16.h), so the step is lane-local
// plus one half-wave exchange.  Every function here is inlined into its caller: no code object holds a symbol of this header.
//
// The rule of visibility.  Row r with causal frontier f (f + 1 = f1) sees the keys c < lim = min(bound, f1) (not causal: bound).
//   * WINDOW, a sliding window of W = window >= 1 keys (include/mfa_window.h): and c >= lo = window_lo(f1, W) = max(f1, W) - W.
//     With span = lim - lo (none: 0) the test is ONE unsigned comparison, c - lo < span.  With W >= column + rows every lo is 0:
//     the plain rule.
//   * SINK, the WINDOW rule with attention sinks (include/mfa_sink.h); window = 0 is "lo = 0 everywhere".
//       - sink TOKENS, sinkTokens = S: the row also sees the keys c < slim = min(S, lim): (c - lo < span) || (c < slim).
//       - sink LOGIT, sinkLogits[query head] (natural units; null: none): one more term of the softmax denominator, s2 = sink log2(e),
//         never scaled by 1 / sqrt(D) or keyScale; L includes it.  A row without a visible key: O = 0, L = s2.
//     With S = 0 and no logits the SINK kernels run the WINDOW kernels' arithmetic in their order.
// A masked score is REPLACED, never multiplied (p = 0 exactly), and the running maximum only ever sees visible keys: a step without
// a visible key keeps m = -FLT_MAX, l = 0, and what a masked key holds -- poison past a length -- never reaches a product.
//
// The rule of the soft cap (CAP; include/mfa_softcap.h).  With raw = q . k and s = raw keyScale / sqrt(D) the natural-unit
// score the softmax sees without a cap (keyScale = 1 for 16-bit caches), a cap > 0 makes it see s' = cap tanh(s / cap) instead.
//   * VISIBLE scores only: a masked score is still replaced, never computed from, so poison past a length never reaches the tanh.
//   * the sink logit is not capped and not scaled; L = log2 of the denominator of the CAPPED scores plus the sink term.
//   * which keys are visible, which tiles are walked, the pieces, the workspace and the O = 0 / L rules of a blind row do not change.
//   * the arithmetic, on the base-2 score the kernels form anyway: with c1 = 2 / cap folded into kscale and c2 = cap log2(e),
//       s2' = c2 (1 - 2 / (1 + exp2(c1 kscale raw))),    exp2(c1 kscale raw) = e^(2 s / cap)
//     -- tanh(x) = 1 - 2 / (1 + e^(2x)) is right at both ends: e^(2x) = +inf gives +c2, 0 gives -c2, never NaN (the form
//     (e^(2x) - 1) / (e^(2x) + 1) is inf / inf there).  One v_exp_f32, one v_rcp_f32 and four plain instructions per score; the
//     cancellation near 0 costs absolute error of the order of c2 2^-24, far below the rounding of P.
//
// The rule of the tree (TREE; include/mfa_tree.h): the new rows of a sequence are the nodes of a speculation tree and see
// their ancestors, not their neighbours in the cache.  With n the keys of the sequence and qn its new rows, P = max(n - qn, 0) is the
// prefix length, node j is key P + j, live = min(qn, n), and row r carries mask_r = masks[b batchStride + r] & (2^live - 1) -- bit j: the
// row sees node j; bits at or past `live` are ignored -- and d_r = max(popcount(mask_r), 1), its depth + 1.  Row r sees key c iff
//   * PREFIX key, c < P: the SINK rule above with the row's frontier at its POSITION P + d_r - 1, not at its index: no window, or
//     c >= lo = window_lo(P + d_r, W), or c < S.
//   * NEW-TOKEN key, P <= c < n: bit c - P of mask_r is set.  The mask alone decides: no causal test and no window test among the new
//     tokens (the host refuses 0 < W < rows, so an ancestor never leaves a descendant's window), and bits j > r are honoured.
//   * everything else is the SINK rule's: a masked score is replaced, a blind row keeps O = 0 / L = -FLT_MAX or the sink logit, the
//     scales and what is never loaded do not change.  The chain mask_r = 2^(r + 1) - 1 is today's causal launch, key for key.
#pragma once
#include "attn_fwd16_common.h"
#include <type_traits>

namespace mfa {

constexpr float STEP_MINUS_HUGE = -3.402823466e+38f;   // m of a row that has seen no key

// the first key a row with frontier f1 - 1 sees under a window of W keys (host range functions and kernels)
template <typename U> __host__ __device__ __forceinline__ U window_lo(U f1, U W) { return (f1 > W ? f1 : W) - W; }

// The keys one query row sees, by the rule above.  `bound`: the keys the launch holds for the row's sequence (decode pieces: their end).
// (CAP changes nothing here: it keeps the capped kernels' instantiations of the step apart from the sink kernels', whose code hipcc
// otherwise orders differently once they share them)
// TREE = 32 / 64: the tree side, with the row's mask in that many bits (decode: M <= 32 rows, the low word; prefill: up to 64 rows);
// `lim` is then the prefix length P, so that the SINK test answers for the prefix keys alone and the mask for the keys from P on.
template <int TREE> struct TreeSide {
  typename std::conditional<TREE == 64, uint64_t, uint32_t>::type mask;
};
template <> struct TreeSide<0> {};
struct TreeRow { uint32_t prefix; uint64_t mask; };   // what the tree kernels construct a row's keys from
template <bool WINDOW, bool SINK, bool CAP = false, int TREE = 0> struct VisibleKeys : TreeSide<TREE> {
  static_assert(!SINK || WINDOW, "the sink kernels are the window kernels plus SINK");
  static_assert(!TREE || (SINK && !CAP && (TREE == 32 || TREE == 64)), "the tree kernels are the sink kernels plus TREE");
  uint32_t lim, lo = 0, span = 0, slim = 0;
  // TREE: row.prefix = P <= bound, row.mask = mask_r (bits at or past `live` already cleared); the frontier is P + d_r
  __device__ __forceinline__ VisibleKeys(uint32_t bound, TreeRow row, uint32_t window, uint32_t sinkTokens) {
    static_assert(TREE != 0, "the constructor of the tree kernels");
    this->mask = (decltype(this->mask))row.mask;
    const uint32_t d = max((uint32_t)__builtin_popcountll(row.mask), 1u);
    lim = min(bound, row.prefix);
    lo = window ? window_lo(row.prefix + d, window) : 0u;
    span = lim > lo ? lim - lo : 0u;
    slim = min(sinkTokens, lim);
  }
  __device__ __forceinline__ VisibleKeys(uint32_t bound, uint32_t f1, uint32_t causal, uint32_t window, uint32_t sinkTokens) {
    lim = bound;
    if (causal) lim = min(lim, f1);
    if constexpr (WINDOW) {
      lo = window_lo(f1, window);
      if constexpr (SINK) lo = window ? lo : 0u;
      span = lim > lo ? lim - lo : 0u;
    }
    if constexpr (SINK) slim = min(sinkTokens, lim);
  }
  __device__ __forceinline__ bool visible(uint32_t c) const {
    if constexpr (TREE != 0) {   // (c < P: j wraps past TREE; c >= P: both prefix tests fail, lim = P)
      const uint32_t j = c - lim;
      return (c - lo < span) | (c < slim) | ((j < (uint32_t)TREE) & (uint32_t)((this->mask >> (j & (uint32_t)(TREE - 1))) & 1u));
    } else if constexpr (SINK) return (c - lo < span) | (c < slim);
    else if constexpr (WINDOW) return c - lo < span;
    else return c < lim;
  }
};

// One online-softmax step of the lane's row over the 32 keys cur .. cur + 31, s[r] the raw score of key cur + crow(r, hi), is three
// calls in this order (three functions that return values, not one that takes m, l, o and P by reference: hipcc allocates the
// bodies' registers as it did with the step written out only in this form):
//   rescale_row(score_max<MASK>(s, keys, cur, hi, kscale), m, l, o);
//   l += score_exp<T, MASK>(s, keys, cur, hi, m, pf);
// MASK false: every key of the step is visible to every row (prefill's unmasked tiles).

// the soft cap of one score: `x` = c1 kscale raw, returns c2 tanh(s / cap) in base-2 units (the rule above)
__device__ __forceinline__ float soft_cap(float x, float c2) {
  return c2 * (1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + fast_exp2(x)));
}

// scales the visible scores (the K scale rides on the softmax scale), replaces the others; returns the row's maximum over the step.
// CAP: `kscale` carries c1 = 2 / cap as well, and the visible scores pass through soft_cap with c2 = `cap2` -- unmasked tiles too
template <bool MASK, bool CAP = false, typename Keys>
__device__ __forceinline__ float score_max(f32x16 &s, const Keys &keys, uint32_t cur, int hi, float kscale, float cap2 = 0.f) {
  float mx = STEP_MINUS_HUGE;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool visible = !MASK || keys.visible(cur + (uint32_t)crow(r, hi));
    if constexpr (CAP) s[r] = visible ? soft_cap(s[r] * kscale, cap2) : STEP_MINUS_HUGE;
    else s[r] = visible ? s[r] * kscale : STEP_MINUS_HUGE;
    mx = fmaxf(mx, s[r]);
  }
  return fmaxf(mx, __shfl_xor(mx, 32));
}

// raises m to the step's maximum: the deferred rescale of l and O
template <int NDB> __device__ __forceinline__ void rescale_row(float mx, float &m, float &l, f32x16 (&o)[NDB]) {
  if (mx > m) {
    const float corr = fast_exp2(m - mx);
    m = mx;
    l *= corr;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= corr;
  }
}

// P = exp2(s - m) in the 16-bit type, as the B operands of vt_mfma for the step's two 16-key halves; returns the row's sum of P
template <typename T, bool MASK, typename Keys>
__device__ __forceinline__ float score_exp(const f32x16 &s, const Keys &keys, uint32_t cur, int hi, float m, typename Frag16<T>::v8 (&pf)[2]) {
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool visible = !MASK || keys.visible(cur + (uint32_t)crow(r, hi));
    const float p = visible ? fast_exp2(s[r] - m) : 0.f;   // replaced, never multiplied
    psum += p;
    pf[r >> 3][r & 7] = (T)p;
  }
  return psum;
}

// tr read: lane n of a 16-lane group supplies row (n>>2), columns 4*(n&3)..+3 of a [4][16] block;
// group (lane>>4): bit0 = d half of the 32-wide d block, bit1 = hi   (dev/attn_fwd16.h)
__device__ __forceinline__ int vtr_lane_offset(int lane, int hi) {
  const int n16 = lane & 15;
  return ((n16 >> 2) + 4 * hi) * 64 + (((lane >> 4) & 1) * 16 + 4 * (n16 & 3)) * 2;
}

// O^T += V^T P^T for 16 keys x 32 d of a V image [D/32][keys][32 d] of 16-bit values: `vp` is the block's first key in the image plus
// the lane's vtr_lane_offset, V^T is gathered by ds_read_b64_tr_b16.  (Returns the accumulator, one call per matrix instruction:
// taking o[] and pf[] by reference moved the bodies' register counts.)
template <typename T> __device__ __forceinline__ f32x16 vt_mfma(const char *vp, typename Frag16<T>::v8 p, f32x16 o) {
  typedef typename Frag16<T>::v8 v8;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp));
  const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(vp + 8 * 64));
  const s16x8 both = __builtin_shufflevector(lo, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
  return Frag16<T>::mfma(__builtin_bit_cast(v8, both), p, o);
}

// The sink logit joins a row's (m, l); returns `fold`, the factor that rescales the row's O with l.  A row without a visible key
// (m = -FLT_MAX, l = 0) ends with m = s2, l = 1.
template <bool CAP = false> __device__ __forceinline__ float fold_sink_logit(float logit, float &m, float &l) {
  float s2 = logit * 1.44269504089f;
  asm volatile("" : "+v"(s2));   // (s2 is the ROUNDED product in m and in both exponents: never fused into the subtractions below)
  const float mnew = fmaxf(m, s2);
  const float fold = fast_exp2(m - mnew);
  l = l * fold + fast_exp2(s2 - mnew);
  m = mnew;
  return fold;
}

// four consecutive values of an O row at element `at`: FP32, or the launch's 16-bit type with its store rounding
template <typename T> __device__ __forceinline__ void store_o4(char *o, int64_t at, bool f32, float4 x) {
  if (f32) *reinterpret_cast<float4 *>(o + at * 4) = x;
  else *reinterpret_cast<u32x2 *>(o + at * 2) = u32x2{pack16<T>(x.x, x.y), pack16<T>(x.z, x.w)};
}

// L = log2 of the row's softmax denominator, m + log2(l); a row without a visible key: -FLT_MAX
__device__ __forceinline__ float row_lse(float m, float l) { return l > 0.f ? m + log2f(l) : STEP_MINUS_HUGE; }

} // namespace mfa
