// attn_mla_index_prefill.h -- the PREFILL indexer (include/mfa_mla_index_prefill.h): the index logits of a prompt chunk of
// any number of rows, and the selection of attn_mla_index.h under prefill's frontier.
//
// LOGITS.  The same product as attn_mla_index.h -- heads on the M side of v_mfma_f32_32x32x16, keys on the N side, the same lane maps and
// the same epilogue chain -- with the OPPOSITE residency: the KEYS stay, the ROWS stream.
//   * split: a workgroup is four waves of ONE sequence, one tile of 256 keys and a SPAN of rows.  Grid: tiles x spans x sequences, tile
//     fastest, so that the workgroups that stream the same rows run together and meet in L2.
//   * B operand: wave w loads the keys tile0 + 64 w + 32 s + q (key sets s = 0, 1) ONCE: lane (q, hi) reads the half row 64 hi .. 64 hi + 63
//     as eight 16-byte loads per set, 2 x 32 registers resident for the whole span.  A key at or past n is zeros and is never loaded; a paged
//     cache reads one table entry per lane and set.
//   * A operand: row r's queries [Hi <= 64][128] and its weights, copied by all 256 threads from global memory into an LDS IMAGE in
//     fragment order: chunk (hb, t, lane) of 16 bytes holds d = 64 hi + 8 t .. + 7 of head 32 hb + q, at ((8 hb + t) 64 + lane) x 16, so
//     that both the copy (thread -> lane tid & 63, t = wave + 4 (j & 1), hb = j >> 1 for its four chunks j) and a wave's read of fragment
//     (hb, t) touch 64 consecutive 16-byte slots: one conflict-free ds_write_b128 / ds_read_b128 per lane.  The 64 weights follow the
//     fragments (heads at or past Hi: zero fragments, weight zero, never loaded).  Two images form a ring: row r + 1 travels global memory
//     -> registers while row r is multiplied, goes to the other image after the products, and ONE barrier ends the row (the image it
//     overwrites was read a row earlier, on the far side of the barrier before).
//   * per row and wave: 8 (Hi <= 32) or 16 fragment reads, each feeding TWO matrix instructions, one per key set, into four f32x16
//     accumulators; then per key set acc = fma(w, max(s, 0), acc) from +0, head block 0 then 1, r ascending, one add across the lane halves,
//     and lanes hi == 0 store 32 contiguous floats masked by c < v(r).  The chain is attn_mla_index.h's: the same 161 roundings.
//   * causal skip: v grows with r, so the span starts at the first row whose prefix reaches the tile, r >= tile0 - max(n - qn, 0); a tile at
//     or past n returns at once; a wave whose 64 keys lie at or past v(r) skips the row's products (it still copies and waits).
//
// SELECT.  mla_index_select_body under MlaipRule: rows counted from the pass's first row, a row at or past queryLengths is all holes.
#pragma once
#include "attn_mla_index.h"

namespace mfa {

constexpr int MLAIP_TILE = 256;                         // keys of a workgroup: 64 a wave, two key sets of 32
constexpr int MLAIP_CHUNKS = 2 * MLAI_NKS * 64;         // 16-byte chunks of a row's fragments
constexpr int MLAIP_IMAGE = MLAIP_CHUNKS + 16;          // ... and its 64 weights, in 16-byte units: 16.25 KiB

struct MlaIndexPrefillArgs : MlaIndexArgs {   // R: the rows of THIS launch (a pass); the logits start at its first row
  const uint32_t *qlengths;   // null: every row is live
  uint32_t rowsAll;           // rows of the chunk
  uint32_t row0;              // the pass's first row
  uint32_t span, spans;       // rows of a span, spans of R
};

// n and qn of a sequence
__device__ __forceinline__ void mlaip_lengths(const MlaIndexPrefillArgs &a, uint32_t batch, uint32_t &n, uint32_t &qn) {
  n = min(a.lengths[batch], a.column);
  qn = a.qlengths ? min(a.qlengths[batch], a.rowsAll) : a.rowsAll;
}

// the prefix [0, v) row `row` (of the chunk) sees: prefill's frontier
__device__ __forceinline__ uint32_t mlaip_prefix(bool causal, uint32_t n, uint32_t qn, uint32_t row) {
  return causal ? min(n, row + (n > qn ? n - qn : 0u) + 1u) : n;
}

struct MlaipRule {
  static __device__ __forceinline__ uint32_t first_row(const MlaIndexPrefillArgs &a) { return a.row0; }
  static __device__ __forceinline__ uint32_t visible(const MlaIndexPrefillArgs &a, uint32_t batch, uint32_t row) {
    uint32_t n, qn;
    mlaip_lengths(a, batch, n, qn);
    return row < qn ? mlaip_prefix(a.causal, n, qn, row) : 0u;
  }
};

template <typename T>
__device__ __forceinline__ void mla_index_prefill_logits_body(const MlaIndexPrefillArgs &a) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  __shared__ u32x4 image[2][MLAIP_IMAGE];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t tile = blockIdx.x % a.tiles, ts = blockIdx.x / a.tiles;
  const uint32_t span = ts % a.spans, batch = ts / a.spans;
  uint32_t n, qn;
  mlaip_lengths(a, batch, n, qn);
  const uint32_t tile0 = tile * (uint32_t)MLAIP_TILE;
  if (tile0 >= n) return;
  // ---- the rows of the span that are live and whose prefix reaches the tile (the same numbers in every thread: the barriers are safe)
  const uint32_t off = n > qn ? n - qn : 0u;
  uint32_t first = a.row0 + span * a.span;
  const uint32_t end = min(min(first + a.span, a.row0 + a.R), qn);
  if (a.causal && tile0 > off) first = max(first, tile0 - off);
  if (first >= end) return;
  const bool two = a.H > 32;   // a second head block

  // ---- the wave's 64 keys, resident for the span; a key at or past n is never loaded
  const int32_t *table = a.table + (int64_t)batch * a.tableStride;
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  const uint32_t key0 = tile0 + 64u * (uint32_t)wave;
  u32x4 kreg[2][MLAI_NKS];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const uint32_t c = key0 + 32u * s + (uint32_t)q;
    const bool valid = c < n;
    int64_t ko = (int64_t)batch * a.bsk + (int64_t)c * a.ldk;
    if (a.paged) ko = (int64_t)(valid ? table[c >> a.pageShift] : 0) * a.psk + (int64_t)(c & pageMask) * a.ldk;
    const char *kp = a.k + (ko + 64 * hi) * 2;
#pragma unroll
    for (int t = 0; t < MLAI_NKS; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (valid) z = *reinterpret_cast<const u32x4 *>(kp + 16 * t);
      kreg[s][t] = z;
    }
  }

  // ---- a row's queries and weights: global memory -> registers (fetch), registers -> an image (stash)
  const char *qbase = a.q + ((int64_t)batch * a.bsq + 64 * hi) * 2;
  const float *wbase = a.w + (int64_t)batch * a.wbs;
  u32x4 pre[4];
  float prew = 0.f;
  auto fetch = [&](uint32_t r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t head = 32u * (j >> 1) + (uint32_t)q;
      const int t = wave + 4 * (j & 1);
      u32x4 z = {0u, 0u, 0u, 0u};
      if (head < a.H) z = *reinterpret_cast<const u32x4 *>(qbase + ((int64_t)head * a.hsq + (int64_t)r * a.ldq) * 2 + 16 * t);
      pre[j] = z;
    }
    if (tid < 64) prew = (uint32_t)tid < a.H ? wbase[(int64_t)r * a.wrs + tid] : 0.f;
  };
  auto stash = [&](int slot) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < 2 || two) image[slot][(8 * (j >> 1) + wave + 4 * (j & 1)) * 64 + lane] = pre[j];
    }
    if (tid < 64) reinterpret_cast<float *>(&image[slot][MLAIP_CHUNKS])[tid] = prew;
  };

  float *out = a.logits + (int64_t)batch * a.lbs;
  fetch(first);
  stash(0);
  __syncthreads();
  int slot = 0;
  for (uint32_t r = first; r < end; ++r) {
    const bool more = r + 1 < end;
    if (more) fetch(r + 1);   // the next row flies under this row's products
    const uint32_t v = mlaip_prefix(a.causal, n, qn, r);
    if (key0 < v) {           // (wave-uniform)
      const u32x4 *img = image[slot];
      f32x16 s[2][2];         // [head block][key set]
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < 16; ++i) s[hb][ks][i] = 0.f;
#pragma unroll
      for (int t = 0; t < MLAI_NKS; ++t) {
        const v8 f = __builtin_bit_cast(v8, img[t * 64 + lane]);
        s[0][0] = F::mfma(f, __builtin_bit_cast(v8, kreg[0][t]), s[0][0]);
        s[0][1] = F::mfma(f, __builtin_bit_cast(v8, kreg[1][t]), s[0][1]);
      }
      if (two) {
#pragma unroll
        for (int t = 0; t < MLAI_NKS; ++t) {
          const v8 f = __builtin_bit_cast(v8, img[(8 + t) * 64 + lane]);
          s[1][0] = F::mfma(f, __builtin_bit_cast(v8, kreg[0][t]), s[1][0]);
          s[1][1] = F::mfma(f, __builtin_bit_cast(v8, kreg[1][t]), s[1][1]);
        }
      }
      // ---- the lane's weights: heads 32 hb + 8 g + 4 hi + (0 .. 3) of group g = r >> 2 are one 16-byte read
      float w[2][16];
#pragma unroll
      for (int hb = 0; hb < 2; ++hb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 x = __builtin_bit_cast(f32x4, img[MLAIP_CHUNKS + 8 * hb + 2 * g + hi]);
#pragma unroll
          for (int i = 0; i < 4; ++i) w[hb][4 * g + i] = x[i];
        }
      float *orow = out + (int64_t)(r - a.row0) * a.lrs;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        // ReLU, weights and the head sum in registers: one rounding per head, then one add across the halves
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = __builtin_fmaf(w[0][i], fmaxf(s[0][ks][i], 0.f), acc);
        if (two) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc = __builtin_fmaf(w[1][i], fmaxf(s[1][ks][i], 0.f), acc);
        }
        const float total = acc + __shfl_xor(acc, 32);
        const uint32_t c = key0 + 32u * ks + (uint32_t)q;
        if (hi == 0 && c < v) orow[c] = total;
      }
    }
    if (more) stash(slot ^ 1);
    __syncthreads();
    slot ^= 1;
  }
}

} // namespace mfa
