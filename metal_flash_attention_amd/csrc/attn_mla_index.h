// attn_mla_index.h -- the MLA sparse indexer (include/mfa_mla_index.h): the index logits of every visible key, and the
// deterministic top-k selection that writes the lists attn_mla16_sparse.h reads.
//
// LOGITS.  logits[b][r][c] = sum_h W[b][r][h] max(q_I[b][h][r] . k_I[b][c], 0).  Per (sequence, row) that is a [Hi <= 64] x [128] by
// [keys] x [128] product on v_mfma_f32_32x32x16 with the HEADS ON THE M SIDE and the KEYS ON THE N SIDE:
//   * A operand: the row's queries.  Lane (q, hi) of head block hb holds head 32 hb + q.  A wave keeps all 2 x 8 fragments (64
//     registers) and its 2 x 16 weights for its whole walk; heads at or past Hi are zeros with weight zero and are never loaded.
//   * B operand: the keys, straight from global memory.  Lane (q, hi) is key key0 + q and reads the HALF ROW 64 hi .. 64 hi + 63 as
//     eight 16-byte loads -- 128 contiguous bytes per lane.  The product sums over d in any order, so k-step t pairs d = 64 hi + 8 t + j
//     of both operands: the same map on the query side, nothing is shuffled.
//   * C: lane (q, hi) owns key column q and the 16 heads 32 hb + crow(r, hi) of each block.  ReLU, the multiply by W and the head sum
//     run in the lane's registers -- acc = fma(w, max(s, 0), acc) from +0, head block 0 then 1, r ascending -- and finish with ONE add
//     across the two lane halves.  No 32-lane reduction, no LDS at all.
//   * split: a workgroup is four waves of ONE (sequence, row); wave w of step s takes the 32 keys tile0 + 32 (4 s + w), `steps` steps.
//     Rows of a sequence do read the same keys, but a wave that served several rows would hold 96 registers of queries and weights
//     per row, or reload them per step; with R = 1 the common case and 256 bytes per key against a 16 KiB query block, each row gets
//     its own workgroup and the grid puts a tile's rows side by side (row fastest) so that their key reads meet in L2.
//   * a tile wholly at or past v returns at once; a lane whose key is at or past v loads nothing (zeros), computes like the others and
//     does not store.
//
// SELECT.  One workgroup of 1024 threads per (sequence, row).  v <= topk: the list is 0 .. v - 1 and holes.  Otherwise a
// most-significant-digit-first radix select over the order-preserving map of the FP32 bits, four passes of 8 bits with a 256-bin
// histogram in LDS (integer counts: the order of the adds cannot show), narrows to the threshold key T and to `want`, the ties at T
// that are admitted; then one ordered pass over [0, v), 4096 positions at a time: ballots give every lane the number of greater keys
// and of ties before it in its wave, the waves' totals meet in LDS, and position i goes to slot greater_before + min(ties_before, want).
// The output is in ascending position, ties go to the lowest positions, and no atomic decides a slot.
#pragma once
#include "attn_fwd16_common.h"

namespace mfa {

constexpr int MLAI_D = 128;            // Di
constexpr int MLAI_STEP = 32;          // keys of a wave's step
constexpr int MLAI_WAVES = 4;          // waves of a logits workgroup
constexpr int MLAI_NKS = 8;            // k-steps of 16
constexpr int MLAI_SELECT_THREADS = 1024;
constexpr int MLAI_SELECT_WAVES = MLAI_SELECT_THREADS / 64;
constexpr uint32_t MLAI_SELECT_UNROLL = 4;   // positions of a thread per round of a pass

struct MlaIndexArgs {
  const char *q;             // QI
  const float *w;            // W
  const char *k;             // KI
  float *logits;
  int32_t *indices;
  const uint32_t *lengths;
  const int32_t *table;
  int64_t tableStride;
  int64_t ldq, hsq, bsq;     // QI; elements
  int64_t ldk, bsk, psk;     // KI
  int64_t wrs, wbs;          // W: row, batch
  int64_t lrs, lbs;          // logits
  int64_t irs, ibs;          // indices
  uint32_t R, H, batches, column, topk;
  uint32_t steps, tiles;     // steps of a wave in a tile; tiles of `column`
  uint32_t pageShift;
  bool paged, causal;
};

// the prefix [0, v) row `row` of sequence `batch` sees
__device__ __forceinline__ uint32_t mlai_visible(const MlaIndexArgs &a, uint32_t batch, uint32_t row) {
  const uint32_t len = min(a.lengths[batch], a.column);
  return a.causal ? min(len, row + (len > a.R ? len - a.R : 0u) + 1u) : len;
}

template <typename T>
__device__ __forceinline__ void mla_index_logits_body(const MlaIndexArgs &a) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t row = blockIdx.x % a.R, bt = blockIdx.x / a.R;
  const uint32_t tile = bt % a.tiles, batch = bt / a.tiles;
  const uint32_t v = mlai_visible(a, batch, row);
  const uint32_t tile0 = tile * (uint32_t)(MLAI_STEP * MLAI_WAVES) * a.steps;
  if (tile0 >= v) return;
  const bool two = a.H > 32;   // a second head block

  // ---- the row's queries and weights, resident for the walk
  v8 qf[2][MLAI_NKS];
  float w[2][16];
  const float *wp = a.w + (int64_t)batch * a.wbs + (int64_t)row * a.wrs;
#pragma unroll
  for (int hb = 0; hb < 2; ++hb) {
    const uint32_t head = 32u * hb + (uint32_t)q;
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head * a.hsq + (int64_t)row * a.ldq + 64 * hi) * 2;
#pragma unroll
    for (int t = 0; t < MLAI_NKS; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (head < a.H) z = *reinterpret_cast<const u32x4 *>(qp + 16 * t);
      qf[hb][t] = __builtin_bit_cast(v8, z);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t h = 32u * hb + (uint32_t)crow(r, hi);
      w[hb][r] = h < a.H ? wp[h] : 0.f;
    }
  }

  const int32_t *table = a.table + (int64_t)batch * a.tableStride;
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  // lane = key c, its half row as the B operand; a key at or past v is never loaded
  auto load_key = [&](uint32_t c, u32x4 (&kreg)[MLAI_NKS]) {
    const bool valid = c < v;
    int64_t ko = (int64_t)batch * a.bsk + (int64_t)c * a.ldk;
    if (a.paged) ko = (int64_t)(valid ? table[c >> a.pageShift] : 0) * a.psk + (int64_t)(c & pageMask) * a.ldk;
    const char *kp = a.k + (ko + 64 * hi) * 2;
#pragma unroll
    for (int t = 0; t < MLAI_NKS; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (valid) z = *reinterpret_cast<const u32x4 *>(kp + 16 * t);
      kreg[t] = z;
    }
  };

  float *out = a.logits + (int64_t)batch * a.lbs + (int64_t)row * a.lrs;
  uint32_t key0 = tile0 + (uint32_t)(MLAI_STEP * wave);
  u32x4 kreg[MLAI_NKS], knext[MLAI_NKS];
  if (key0 < v) load_key(key0 + (uint32_t)q, kreg);
  for (uint32_t s = 0; s < a.steps && key0 < v; ++s) {   // (wave-uniform; the kernel has no barrier)
    const uint32_t after = key0 + (uint32_t)(MLAI_STEP * MLAI_WAVES);
    const bool more = s + 1 < a.steps && after < v;
    if (more) load_key(after + (uint32_t)q, knext);      // the next step's rows fly under this step's products
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) s0[r] = s1[r] = 0.f;
#pragma unroll
    for (int t = 0; t < MLAI_NKS; ++t) s0 = F::mfma(qf[0][t], __builtin_bit_cast(v8, kreg[t]), s0);
    if (two) {
#pragma unroll
      for (int t = 0; t < MLAI_NKS; ++t) s1 = F::mfma(qf[1][t], __builtin_bit_cast(v8, kreg[t]), s1);
    }
    // ---- ReLU, weights and the head sum in registers: one rounding per head, then one add across the halves
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = __builtin_fmaf(w[0][r], fmaxf(s0[r], 0.f), acc);
    if (two) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc = __builtin_fmaf(w[1][r], fmaxf(s1[r], 0.f), acc);
    }
    const float total = acc + __shfl_xor(acc, 32);
    const uint32_t c = key0 + (uint32_t)q;
    if (hi == 0 && c < v) out[c] = total;
    if (more) {
#pragma unroll
      for (int t = 0; t < MLAI_NKS; ++t) kreg[t] = knext[t];
    }
    key0 = after;
  }
}

// the total order of FP32 bit patterns as unsigned keys: larger logit, larger key; -0 < +0
__device__ __forceinline__ uint32_t mlai_order_key(float x) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, x);
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// The select kernel's visibility rule: which row of the launch a workgroup's local row is (first_row + local; the logits of a launch
// start at its first row, the lists at row 0) and the prefix that row sees.  This one is the decode indexer's; the prefill indexer's
// (attn_mla_index_prefill.h) counts rows from a pass's first row and gives a row at or past queryLengths the prefix 0: all holes, no
// logit read.
struct MlaiDecodeRule {
  static __device__ __forceinline__ uint32_t first_row(const MlaIndexArgs &) { return 0u; }
  static __device__ __forceinline__ uint32_t visible(const MlaIndexArgs &a, uint32_t batch, uint32_t row) { return mlai_visible(a, batch, row); }
};

template <typename Rule, typename Args>
__device__ __forceinline__ void mla_index_select_body(const Args &a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pick[2];                          // the pass's digit; what is still wanted inside it
  __shared__ uint32_t totals[2][MLAI_SELECT_UNROLL * MLAI_SELECT_WAVES];   // per (u, wave): greater | ties << 16, double buffered
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t local = blockIdx.x % a.R, batch = blockIdx.x / a.R, row = Rule::first_row(a) + local;
  const uint32_t v = Rule::visible(a, batch, row), topk = a.topk;
  const float *x = a.logits + (int64_t)batch * a.lbs + (int64_t)local * a.lrs;
  int32_t *out = a.indices + (int64_t)batch * a.ibs + (int64_t)row * a.irs;

  if (v <= topk) {   // every visible position, then holes: no logit is read
    for (uint32_t i = tid; i < topk; i += MLAI_SELECT_THREADS) out[i] = i < v ? (int32_t)i : -1;
    return;
  }

  // ---- the threshold key, most significant digit first: `prefix` under `mask` is what a candidate's key starts with, `want` how many
  // of the candidates are taken (>= 1, and fewer than there are candidates or all of them)
  uint32_t prefix = 0, mask = 0, want = topk;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (uint32_t i0 = tid; i0 < v; i0 += MLAI_SELECT_UNROLL * MLAI_SELECT_THREADS) {   // the unroll's loads fly together
      float xv[MLAI_SELECT_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < MLAI_SELECT_UNROLL; ++u) {
        const uint32_t i = i0 + u * MLAI_SELECT_THREADS;
        xv[u] = i < v ? x[i] : 0.f;
      }
#pragma unroll
      for (uint32_t u = 0; u < MLAI_SELECT_UNROLL; ++u) {
        const uint32_t key = mlai_order_key(xv[u]);
        if (i0 + u * MLAI_SELECT_THREADS < v && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (wave == 0) {   // lane: bins 4 lane .. 4 lane + 3; `above` counts the candidates of higher bins
      uint32_t c[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) tot += c[j] = hist[4 * lane + j];
      uint32_t suffix = tot;
#pragma unroll
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_down(suffix, d);
        if (lane + d < 64) suffix += t;
      }
      uint32_t above = suffix - tot;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (above < want && want <= above + c[j]) {   // true for exactly one bin
          pick[0] = 4 * lane + j;
          pick[1] = want - above;
        }
        above += c[j];
      }
    }
    __syncthreads();
    prefix |= pick[0] << shift;
    mask |= 0xFFu << shift;
    want = pick[1];
  }

  // ---- the ordered pass: keys above the threshold, and the first `want` ties, in ascending position.  A round takes UNROLL x 1024
  // positions; thread t holds positions i0 + 1024 u + t, so the round's order is (u, wave, lane)
  uint32_t greaterBase = 0, tieBase = 0, buf = 0;
  const uint64_t lower = (1ull << lane) - 1ull;
  for (uint32_t i0 = 0; i0 < v; i0 += MLAI_SELECT_UNROLL * MLAI_SELECT_THREADS) {
    float xv[MLAI_SELECT_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < MLAI_SELECT_UNROLL; ++u) {
      const uint32_t i = i0 + u * MLAI_SELECT_THREADS + tid;
      xv[u] = i < v ? x[i] : 0.f;
    }
    bool greater[MLAI_SELECT_UNROLL], tie[MLAI_SELECT_UNROLL];
    uint32_t gBefore[MLAI_SELECT_UNROLL], tBefore[MLAI_SELECT_UNROLL];   // first: inside the wave
#pragma unroll
    for (uint32_t u = 0; u < MLAI_SELECT_UNROLL; ++u) {
      const bool in = i0 + u * MLAI_SELECT_THREADS + tid < v;
      const uint32_t key = mlai_order_key(xv[u]);
      greater[u] = in && key > prefix;
      tie[u] = in && key == prefix;
      const uint64_t gb = __ballot(greater[u]), tb = __ballot(tie[u]);
      gBefore[u] = (uint32_t)__popcll(gb & lower);
      tBefore[u] = (uint32_t)__popcll(tb & lower);
      if (lane == 0) totals[buf][u * MLAI_SELECT_WAVES + wave] = (uint32_t)__popcll(gb) | ((uint32_t)__popcll(tb) << 16);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t at = 0; at < MLAI_SELECT_UNROLL * MLAI_SELECT_WAVES; ++at) {   // (at / WAVES is a constant: the arrays stay registers)
      if (at % MLAI_SELECT_WAVES == wave) {
        gBefore[at / MLAI_SELECT_WAVES] += greaterBase;
        tBefore[at / MLAI_SELECT_WAVES] += tieBase;
      }
      const uint32_t t = totals[buf][at];
      greaterBase += t & 0xFFFFu;
      tieBase += t >> 16;
    }
#pragma unroll
    for (uint32_t u = 0; u < MLAI_SELECT_UNROLL; ++u) {
      const uint32_t slot = gBefore[u] + min(tBefore[u], want);
      if ((greater[u] || (tie[u] && tBefore[u] < want)) && slot < topk) out[slot] = (int32_t)(i0 + u * MLAI_SELECT_THREADS + tid);
    }
    buf ^= 1u;
    if (greaterBase + min(tieBase, want) >= topk) break;   // the list is full (the same numbers in every thread)
  }
}

} // namespace mfa
