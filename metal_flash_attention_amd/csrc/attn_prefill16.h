// attn_prefill16.h -- prefill attention over a KV cache on the 16-bit matrix cores of gfx950: a block of new query rows per sequence
// against keys that already live in a 16-bit or FP8 (e4m3), contiguous or paged cache (include/mfa_prefill.h).
// Compiler-scheduled HIP built from what attn_decode16.h and attn_fwd16_v3.h have proven:
//   * PACKING, decode's idea widened: one workgroup of 4 waves owns 128 packed rows of ONE K / V head of one sequence -- RB = 128 / G
//     consecutive query rows for each of the G query heads of the group -- so K and V are read once per group, not G times.  Packed row
//     p < G RB is head kvh G + p / RB, row r0 + p % RB; wave w owns packed rows 32 w .. 32 w + 31; rows >= G RB (G = 3: 126, 127) and
//     rows at or past the sequence's queryLengths repeat the last live one and store nothing.
//   * the fragment maps of dev/attn_fwd16.h: S^T = K Q^T with v_mfma_f32_32x32x16, a lane owns one packed row (frontier, running
//     (m, l) and the rescale are lane-local plus one half-wave exchange), P converted in registers is the B operand of O^T += V^T P^T.
//     Q fragments stay in registers (D/16 x 4 VGPRs), O^T is D/32 x 16 accumulators.
//   * K and V go through LDS, shared by the four waves (every wave needs every key): tiles of 64 keys, double-buffered; a row-major K
//     image XOR-swizzled by kswz (attn_fwd16_common.h) and read as A fragments with ds_read_b128, and the V image [D/32][64 keys][32 d]
//     gathered as V^T by ds_read_b64_tr_b16 exactly as attn_decode16.h does.  Staged through registers (global load -> VGPR ->
//     ds_write): the loads of tile t + 1 are issued before tile t is computed and written to the other buffer after it, one barrier
//     per tile.
//   * FP8 is one template parameter: the e4m3 bytes are converted in the staging registers (cvt8_e4m3, kv_e4m3.h: exact) between
//     the load and the LDS write.  From the LDS images on the two kernels are the same code, with no permuted contraction: on exactly
//     convertible values the e4m3 and the 16-bit launch are byte-identical.
//   * keys are addressed in groups of 16 (a tile starts on a multiple of 64 and a page holds at least 16 keys, so a group never
//     straddles a page): four wave-uniform block-table reads per tile, none per lane.  The contiguous layout takes the same path with
//     the batch stride in place of the page, so paged and contiguous launches run the same arithmetic in the same order.
//   * prefill_tile_range -- one function, device and host (mfa_attention_prefill_tile_range) -- gives the block its tiles: [0,
//     first_masked) run without the per-element mask, [first_masked, end) with it, tiles at or past end are never loaded.
//   * what may hold poison is never loaded: key rows at or past n come in as zeros (K and V), a masked score is REPLACED (p = 0 exactly),
//     and the running maximum only ever sees visible keys -- a row without a visible key keeps m = -FLT_MAX, l = 0.
//   * D = 256: the same body at one workgroup per compute unit (128 KiB of LDS); over a 16-bit cache an instruction of
//     the workgroup covers eight rows, half a 16-key group, and the staging addresses follow (RPI below).
//
// WINDOW, SINK: the rule of which keys a row sees, and the sink logit, are attn_cache_step.h's.  What is prefill's own:
//   * WINDOW: prefill_window_tile_range gives the block four tile indices: [begin, unmaskedBegin) runs with the per-element mask (a
//     row's window starts inside), [unmaskedBegin, unmaskedEnd) without, [unmaskedEnd, end) with it again (causal frontiers and n);
//     tiles outside [begin, end) are never loaded -- no key, no page, no block-table entry.  The first load is tile `begin`, the
//     buffer of tile t is (t - begin) & 1.  With W >= column + rows: begin = unmaskedBegin = 0, unmaskedEnd = first_masked.
//   * SINK tokens: prefill_sink_tile_range adds a fifth index: a fourth loop walks the tiles [0, sinkEnd) AHEAD of the three that
//     exist, always with the per-element mask; sinkEnd <= begin, and the tiles between them are never loaded.  The buffer of a tile
//     is its POSITION in the walked list [0, sinkEnd) ++ [begin, end), not t - begin.  Every masked tile tests the whole rule, so
//     sink keys inside the window's own masked tiles (S reaches `begin`: the zones touch) are seen as well.
//   * SINK logit: joins (m, l) at the normalisation.
//
// CAP: the soft cap of attn_cache_step.h on the visible scores of every tile, the unmasked ones included; the SINK body otherwise (any
// window and sinks, none included; RAGGED or not): c1 rides on kscale, c2 goes to score_max.
//
// TREE: the tree rule of attn_cache_step.h, the SINK body otherwise (any window and sinks, none included; not RAGGED, no CAP).  The lane's
// mask is that of its ROW `row` -- never of its packed index; lanes that repeat the last live row read that row's mask, rows at or past qn
// are never read.  A row's mask may name any new token and its depth is not its index, so every row block of a sequence walks the SAME
// tiles, prefill_tree_tile_range's, through the four loops that exist: the tiles an earlier row block walks beyond its causal end are
// fully masked for a chain (p = 0, the row maximum untouched, +0 added) and change no bit.
//
// SPLIT (include/mfa_split.h): the launch cut along the keys, the SINK or the TREE body otherwise (any window and sinks,
// none included; not RAGGED, no CAP).  The grid gains a piece index, the fastest: the pieces of one block are neighbours and share Q.
//   * piece i of P of a block takes the positions [i W / P, (i + 1) W / P) of THAT BLOCK'S OWN walked list [0, sinkEnd) ++ [beginTile,
//     endTile): prefill_split_piece_range -- one function, device and host (mfa_attention_prefill_split_piece_range) -- NARROWS the
//     block's five indices to the piece, and the four loops, the first load and the buffer of a tile (its position inside the piece) are
//     the unsplit body's on the narrowed indices.  Whether a tile runs with the per-element mask stays a property of the tile.
//   * a live row publishes its un-normalised O (FP32, 16 bytes per lane straight from the accumulators) and (m, l) to the piece's slab
//     wsO[piece][b][head][row][D], wsML[piece][b][head][row][2]; a piece that walked no tile still publishes (-FLT_MAX, 0), and a row
//     whose l is 0 leaves its O slab alone.  Rows at or past queryLengths[b] and blocks without a live row write nothing.
//   * the sink logit and the value scale are NOT the pieces' business: prefill16_combine_body, which has the head index, merges a row's
//     pieces by the weights exp2(m_s - m*), reads a piece's O only where its l > 0, and THEN folds the sink logit and applies the value
//     scale -- each exactly once per row, also when piece 0 is empty.  (Decode's "piece 0 folds" was the alternative.)
#pragma once
#include "attn_cache_step.h"
#include "kv_e4m3.h"
#include <type_traits>

#define MFA_PREFILL_INLINE __attribute__((always_inline))   // (tile-load lambdas forced inline: see the top of attn_fwd16_v3.h)

namespace mfa {

constexpr int PF_TILE = 64;      // keys per tile (MFA_PREFILL_KEY_TILE)
constexpr int PF_ROWS = 128;     // packed rows per workgroup (MFA_PREFILL_PACKED_ROWS)
constexpr int PF_THREADS = 256;

struct PrefillArgs {
  const char *q, *k, *v;
  char *o;
  float *l;                       // null: not stored
  const uint32_t *lengths;
  const uint32_t *qlengths;       // null: every sequence has `rows`
  const int32_t *table;           // paged launches
  int64_t tableStride;
  int64_t ldq, hsq, bsq;          // elements
  int64_t ldk, hsk, bsk, psk;
  int64_t ldv, hsv, bsv, psv;
  int64_t ldo, hso, bso;
  int64_t lhs, lbs;
  const float *keyScale, *valueScale;   // null: 1.0
  uint32_t rows, G, RB, rowBlocks, Hkv, batches, column;
  uint32_t paged, pageShift;      // pageSize = 1 << pageShift
  uint32_t causal, outF32;
  float scale2;                   // log2(e) / sqrt(D)
  uint32_t window;                // the WINDOW kernels only (>= 1); last, so that no other field moves
  uint32_t sinkTokens;            // the SINK kernels only, which also take window = 0 (no window); behind `window` in turn
  const float *sinkLogits;        // [heads], natural units; null: none
  const uint32_t *rowStarts;      // the RAGGED kernels only: [batches + 1], packed rows (include/mfa_ragged.h); behind the sinks in turn
  uint32_t totalRows, slots;      // T; the slots of the grid (`rowBlocks` stays ceil(rows / RB))
  float capIn, capOut;            // the CAP kernels only: c1 = 2 / cap and c2 = cap log2(e) (attn_cache_step.h); behind the ragged fields in turn
  const uint64_t *masks;          // the TREE kernels only: [batches][rows] row masks (include/mfa_tree.h); last in turn
  int64_t maskStride;             // elements between two sequences' masks; 0: one tree for all
  uint32_t pieces, heads;         // the SPLIT kernels and the combine kernel only: P >= 2, and Hq = Hkv G; last in turn
  float *wsO, *wsML;              // the slabs of include/mfa_split.h
};

// The tiles of the block of rows [r0, r0 + RB) of a sequence of n keys and qn rows.  Row r sees keys c < lim(r) = n, or with `causal`
// min(n, r + max(n - qn, 0) + 1): *end = ceil(lim(last live row) / 64), *firstMasked = floor(lim(r0) / 64) -- below it every key of a
// tile is visible to every live row.  Device and host (mfa_attention_prefill_tile_range) run this one body.
__host__ __device__ __forceinline__ void prefill_tile_range(uint32_t n, uint32_t qn, uint32_t r0, uint32_t RB, uint32_t causal,
                                                            uint32_t *firstMasked, uint32_t *end) {
  if (r0 >= qn || n == 0) {
    *firstMasked = *end = 0;
    return;
  }
  uint64_t lo = n, hi = n;
  if (causal) {
    const uint64_t off = n > qn ? (uint64_t)n - qn : 0;
    uint64_t last = (uint64_t)r0 + RB;
    if (last > qn) last = qn;
    lo = (uint64_t)r0 + off + 1;
    hi = last + off;   // (last - 1) + off + 1
    if (lo > n) lo = n;
    if (hi > n) hi = n;
  }
  const uint64_t e = (hi + PF_TILE - 1) / PF_TILE;
  uint64_t f = lo / PF_TILE;
  if (f > e) f = e;
  *firstMasked = (uint32_t)f;
  *end = (uint32_t)e;
}

// The same under a window of `window` >= 1 keys (causal): row r sees lo(r) <= c < lim(r) with f1 = r + max(n - qn, 0) + 1,
// lim = min(n, f1), lo = max(f1, window) - window; both grow with r.  *begin = floor(lo(r0) / 64), *end = ceil(lim(last live row) / 64):
// the tightest range that holds every visible key.  [*unmaskedBegin, *unmaskedEnd) = [ceil(lo(last) / 64), floor(lim(r0) / 64)): the
// tiles whose every key every live row sees; empty: both = *begin.  A block without a live row or without a visible key: all 0.
// Device and host (mfa_attention_prefill_window_tile_range) run this one body.
__host__ __device__ __forceinline__ void prefill_window_tile_range(uint32_t n, uint32_t qn, uint32_t r0, uint32_t RB, uint32_t window,
                                                                   uint32_t *begin, uint32_t *unmaskedBegin, uint32_t *unmaskedEnd,
                                                                   uint32_t *end) {
  *begin = *unmaskedBegin = *unmaskedEnd = *end = 0;
  if (r0 >= qn || n == 0) return;
  const uint64_t off = n > qn ? (uint64_t)n - qn : 0, W = window;
  uint64_t last = (uint64_t)r0 + RB;
  if (last > qn) last = qn;
  const uint64_t f1First = (uint64_t)r0 + off + 1, f1Last = last + off;
  const uint64_t loFirst = window_lo(f1First, W), loLast = window_lo(f1Last, W);
  if (loFirst >= n) return;   // (n < qn: the window of the block's first row, and of every later one, lies past the keys)
  const uint64_t limFirst = f1First < n ? f1First : n, limLast = f1Last < n ? f1Last : n;
  const uint64_t b = loFirst / PF_TILE, e = (limLast + PF_TILE - 1) / PF_TILE;
  uint64_t u0 = (loLast + PF_TILE - 1) / PF_TILE, u1 = limFirst / PF_TILE;
  if (u0 >= u1) u0 = u1 = b;
  *begin = (uint32_t)b;
  *unmaskedBegin = (uint32_t)u0;
  *unmaskedEnd = (uint32_t)u1;
  *end = (uint32_t)e;
}

// The same with `sinkTokens` sink keys (window = 0: no window, and then no sink keys -- prefill_tile_range's two indices under `causal`
// with begin = unmaskedBegin = 0).  *sinkEnd = min(ceil(min(S, lim(last live row)) / 64), *begin): the tiles [0, *sinkEnd) are walked
// ahead of [*begin, *end), with the per-element mask.  A block whose rows all lie past their window's keys (n < qn) sees its sink keys
// alone: all five = ceil(min(S, n) / 64).  Device and host (mfa_attention_prefill_sink_tile_range) run this one body.
__host__ __device__ __forceinline__ void prefill_sink_tile_range(uint32_t n, uint32_t qn, uint32_t r0, uint32_t RB, uint32_t causal,
                                                                 uint32_t window, uint32_t sinkTokens, uint32_t *begin,
                                                                 uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end,
                                                                 uint32_t *sinkEnd) {
  *begin = *unmaskedBegin = *unmaskedEnd = *end = *sinkEnd = 0;
  if (r0 >= qn || n == 0) return;
  if (!window) {
    prefill_tile_range(n, qn, r0, RB, causal, unmaskedEnd, end);
    return;
  }
  prefill_window_tile_range(n, qn, r0, RB, window, begin, unmaskedBegin, unmaskedEnd, end);
  if (!sinkTokens) return;
  if (*end == 0) {   // no row of the block sees a key of its window: lim = n for every row
    const uint64_t sunk = sinkTokens < n ? sinkTokens : n;
    *begin = *unmaskedBegin = *unmaskedEnd = *end = *sinkEnd = (uint32_t)((sunk + PF_TILE - 1) / PF_TILE);
    return;
  }
  const uint64_t off = n > qn ? (uint64_t)n - qn : 0;
  uint64_t last = (uint64_t)r0 + RB;
  if (last > qn) last = qn;
  uint64_t limLast = last + off;
  if (limLast > n) limLast = n;
  const uint64_t sunk = sinkTokens < limLast ? sinkTokens : limLast;
  const uint64_t tiles = (sunk + PF_TILE - 1) / PF_TILE;
  *sinkEnd = tiles < *begin ? (uint32_t)tiles : *begin;
}

// TREE (include/mfa_tree.h): the tiles EVERY row block of a sequence of n keys and qn rows walks under a speculation tree.  With P =
// max(n - qn, 0), live = min(qn, n) and lo(f) = window ? max(f, window) - window : 0, a node's frontier lies in [P + 1, P + live]:
//   *begin = floor(lo(P + 1) / 64), *end = ceil(n / 64): the tightest range that holds every key any row can see through its window;
//   [*unmaskedBegin, *unmaskedEnd) = [ceil(lo(P + live) / 64), floor(P / 64)): the tiles whose every key is a prefix key inside every
//   row's window -- key P itself is a tree key and masked; empty: both = *begin;
//   *sinkEnd = min(ceil(min(S, P) / 64), *begin): the sink tiles walked ahead, with the per-element mask.
// n = 0 or qn = 0: all 0.  Device and host (mfa_attention_prefill_tree_tile_range) run this one body.
__host__ __device__ __forceinline__ void prefill_tree_tile_range(uint32_t n, uint32_t qn, uint32_t window, uint32_t sinkTokens, uint32_t *begin,
                                                                 uint32_t *unmaskedBegin, uint32_t *unmaskedEnd, uint32_t *end, uint32_t *sinkEnd) {
  *begin = *unmaskedBegin = *unmaskedEnd = *end = *sinkEnd = 0;
  if (n == 0 || qn == 0) return;
  const uint64_t P = n > qn ? (uint64_t)n - qn : 0, live = qn < n ? qn : n, W = window;
  const uint64_t loFirst = W ? window_lo(P + 1, W) : 0, loLast = W ? window_lo(P + live, W) : 0;
  const uint64_t b = loFirst / PF_TILE, e = ((uint64_t)n + PF_TILE - 1) / PF_TILE;
  uint64_t u0 = (loLast + PF_TILE - 1) / PF_TILE, u1 = P / PF_TILE;
  if (u0 >= u1) u0 = u1 = b;
  const uint64_t sunk = sinkTokens < P ? sinkTokens : P;
  const uint64_t tiles = (sunk + PF_TILE - 1) / PF_TILE;
  *begin = (uint32_t)b;
  *unmaskedBegin = (uint32_t)u0;
  *unmaskedEnd = (uint32_t)u1;
  *end = (uint32_t)e;
  *sinkEnd = (uint32_t)(tiles < b ? tiles : b);
}

// SPLIT (include/mfa_split.h): piece `piece` of `pieces` of the walked list [0, sinkEnd) ++ [beginTile, endTile) of W tiles takes the
// positions [piece W / pieces, (piece + 1) W / pieces): the tiles [begin[0], end[0]) inside the sink tiles, then [begin[1], end[1])
// inside [beginTile, endTile) -- decode_sink_piece_range's arithmetic, on tiles.  sinkEnd <= beginTile <= endTile.  Device and host
// (mfa_attention_prefill_split_piece_range) run this one body.
__host__ __device__ __forceinline__ void prefill_split_piece_range(uint32_t beginTile, uint32_t endTile, uint32_t sinkEnd, uint32_t pieces,
                                                                   uint32_t piece, uint32_t *begin, uint32_t *end) {
  const uint32_t tiles = sinkEnd + (endTile - beginTile);
  const uint32_t t0 = (uint32_t)((uint64_t)piece * tiles / pieces), t1 = (uint32_t)(((uint64_t)piece + 1) * tiles / pieces);   // positions in the list
  begin[0] = t0 < sinkEnd ? t0 : sinkEnd;
  end[0] = t1 < sinkEnd ? t1 : sinkEnd;
  begin[1] = beginTile + (t0 > sinkEnd ? t0 - sinkEnd : 0u);
  end[1] = beginTile + (t1 > sinkEnd ? t1 - sinkEnd : 0u);
}

// RAGGED (include/mfa_ragged.h): which row block slot `slot` of a launch over packed rows serves.  Sequence b owns the packed rows
// [s_b, s_b + qn_b), s_b = min(starts[b], T), e_b = min(starts[b + 1], T), qn_b = min(max(e_b - s_b, 0), rows), in ceil(qn_b / RB) row
// blocks; the slots count the row blocks of sequence 0, then those of sequence 1, ...  *sequence = UINT32_MAX: a slot past the total.
// This scalar walk is the DEFINITION and what the host runs (mfa_attention_prefill_ragged_block); the kernels run
// prefill_ragged_block_wave below, which returns its answer.  (sum_b ceil(qn_b / RB) <= batches x ceil(rows / RB) <= 2^31 - 1: the
// host has checked it, nothing wraps.)
__host__ __device__ __forceinline__ uint32_t prefill_ragged_count(uint32_t start, uint32_t next, uint32_t T, uint32_t rows, uint32_t *s) {
  const uint32_t a = start < T ? start : T, e = next < T ? next : T;
  *s = a;
  const uint32_t span = e > a ? e - a : 0u;
  return span < rows ? span : rows;
}
__host__ __device__ __forceinline__ void prefill_ragged_block(const uint32_t *starts, uint32_t batches, uint32_t T, uint32_t rows,
                                                              uint32_t RB, uint32_t slot, uint32_t *sequence, uint32_t *firstRow,
                                                              uint32_t *start, uint32_t *count) {
  uint32_t before = 0;
  for (uint32_t b = 0; b < batches; ++b) {
    uint32_t s;
    const uint32_t qn = prefill_ragged_count(starts[b], starts[b + 1], T, rows, &s);
    const uint32_t nb = qn / RB + (qn % RB != 0);
    if (slot - before < nb) {
      *sequence = b; *firstRow = (slot - before) * RB; *start = s; *count = qn;
      return;
    }
    before += nb;
  }
  *sequence = 0xffffffffu; *firstRow = 0; *start = 0; *count = 0;
}

#if defined(__HIPCC__)
// The same answer, 64 sequences at a time: lane i of every wave takes sequence base + i, an inclusive prefix sum over the wave gives
// the slots at or before each sequence, and the first lane whose sum passes `slot` holds the sequence.  All results wave-uniform.
__device__ __forceinline__ void prefill_ragged_block_wave(const uint32_t *starts, uint32_t batches, uint32_t T, uint32_t rows, uint32_t RB,
                                                          uint32_t slot, int lane, uint32_t *sequence, uint32_t *firstRow, uint32_t *start,
                                                          uint32_t *count) {
  uint32_t before = 0;
  *sequence = 0xffffffffu; *firstRow = 0; *start = 0; *count = 0;
  for (uint32_t base = 0; base < batches; base += 64u) {
    const uint32_t b = base + (uint32_t)lane;
    uint32_t s = 0, qn = 0;
    if (b < batches) qn = prefill_ragged_count(starts[b], starts[b + 1], T, rows, &s);
    const uint32_t nb = qn / RB + (qn % RB != 0);
    uint32_t incl = nb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
      if (lane >= d) incl += up;
    }
    const unsigned long long hit = __ballot(before + incl > slot);
    if (hit) {
      const int first = __builtin_ctzll(hit);
      const uint32_t blocksBefore = before + (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)(incl - nb), first));
      *sequence = base + (uint32_t)first;
      *firstRow = (slot - blocksBefore) * RB;
      *start = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)s, first));
      *count = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)qn, first));
      return;
    }
    before += (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)incl, 63));
  }
}
#endif

template <int D> constexpr int prefill16_lds_bytes() { return 2 /*buffers*/ * 2 /*K, V*/ * PF_TILE * D * 2; }

template <typename T, int D, bool FP8, bool WINDOW = false, bool SINK = false, bool RAGGED = false, bool CAP = false, bool TREE = false,
          bool SPLIT = false>
__device__ __forceinline__ void prefill16_body(const PrefillArgs &a) {
  static_assert(!TREE || (SINK && !RAGGED && !CAP), "the tree kernels are the sink kernels plus TREE");
  static_assert(!SPLIT || (SINK && !RAGGED && !CAP), "the split kernels are the sink or the tree kernels plus SPLIT");
  static_assert(!RAGGED || SINK, "the ragged kernels are the sink kernels plus RAGGED");
  static_assert(!CAP || SINK, "the capped kernels are the sink kernels plus CAP");
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NDB = D / 32, NKS = D / 16;
  constexpr int ROWB = D * 2, KIMG = PF_TILE * ROWB, VIMG = PF_TILE * D * 2, STAGE = KIMG + VIMG;
  constexpr int ESZ = FP8 ? 1 : 2;                // bytes of a cache element
  constexpr int CPR = D * ESZ / 16;               // 16-byte chunks of a cache row
  constexpr int RPI = PF_THREADS / CPR;           // rows one workgroup-instruction covers
  constexpr int NCH = PF_TILE / RPI;              // chunks per thread, per operand, per tile
  static_assert(PF_TILE % RPI == 0 && NCH >= 1, "a tile divides evenly over the workgroup");

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;

  // ---- the block: (row block, K / V head, sequence); the blocks of one (sequence, K / V head) are neighbours on one XCD
  uint32_t rb, kvh, batch;
  const uint32_t RB = a.RB;
  uint32_t r0, qn, packed = 0;   // RAGGED: `packed` = s_b, the sequence's first packed row; Q, O and L have no batch axis
  if constexpr (RAGGED) {
    // the grid is slots x K / V heads: (slot, K / V head) come out of the same XCD-aware order, the slot gives (sequence, row block)
    const Fwd16Grid g{a.slots, a.Hkv, 1u, 1u, nullptr, nullptr};
    fwd16_decode_block(g, blockIdx.x, &rb, &kvh, &batch);
    if (a.causal) rb = a.slots - 1 - rb;   // (the order of the slots is free: the last sequences' last row blocks start first)
    prefill_ragged_block_wave(a.rowStarts, a.batches, a.totalRows, a.rows, RB, rb, lane, &batch, &r0, &packed, &qn);
    if (batch == 0xffffffffu) return;      // a slot past the total: nothing is read or written
  } else {
    const Fwd16Grid g{a.rowBlocks, a.Hkv, a.batches, 1u, nullptr, nullptr};
    fwd16_decode_block(g, SPLIT ? blockIdx.x / a.pieces : blockIdx.x, &rb, &kvh, &batch);   // (SPLIT: the piece is the fastest index)
    if (a.causal) rb = a.rowBlocks - 1 - rb;   // later row blocks traverse more keys: start them first
    qn = a.qlengths ? min(a.qlengths[batch], a.rows) : a.rows;
    r0 = rb * RB;
  }
  const uint32_t n = min(a.lengths[batch], a.column);
  if (r0 >= qn) return;   // no live row: nothing is read or written
  uint32_t firstMasked, endTile, beginTile = 0, unmaskedBegin = 0;   // (WINDOW: firstMasked is unmaskedEnd)
  uint32_t sinkEnd = 0;   // SINK: the tiles [0, sinkEnd) are walked ahead of [beginTile, endTile)
  if constexpr (TREE) prefill_tree_tile_range(n, qn, a.window, a.sinkTokens, &beginTile, &unmaskedBegin, &firstMasked, &endTile, &sinkEnd);
  else if constexpr (SINK) prefill_sink_tile_range(n, qn, r0, RB, a.causal, a.window, a.sinkTokens, &beginTile, &unmaskedBegin, &firstMasked, &endTile, &sinkEnd);
  else if constexpr (WINDOW) prefill_window_tile_range(n, qn, r0, RB, a.window, &beginTile, &unmaskedBegin, &firstMasked, &endTile);
  else prefill_tile_range(n, qn, r0, RB, a.causal, &firstMasked, &endTile);
  // SPLIT: the five indices narrowed to the piece -- its sink tiles are [sinkBegin, sinkEnd), its other tiles [beginTile, endTile), of
  // which [unmaskedBegin, firstMasked) run without the per-element mask; all wave-uniform, kept in scalar registers
  uint32_t sinkBegin = 0;
  if constexpr (SPLIT) {
    uint32_t pb[2], pe[2];
    prefill_split_piece_range(beginTile, endTile, sinkEnd, a.pieces, blockIdx.x % a.pieces, pb, pe);
    sinkBegin = (uint32_t)__builtin_amdgcn_readfirstlane((int)pb[0]);
    sinkEnd = (uint32_t)__builtin_amdgcn_readfirstlane((int)pe[0]);
    beginTile = (uint32_t)__builtin_amdgcn_readfirstlane((int)pb[1]);
    endTile = (uint32_t)__builtin_amdgcn_readfirstlane((int)pe[1]);
    unmaskedBegin = min(max(unmaskedBegin, beginTile), endTile);
    firstMasked = min(max(firstMasked, beginTile), endTile);
  }
  float kscale = a.scale2 * (a.keyScale ? a.keyScale[kvh] : 1.0f);
  if constexpr (CAP) kscale *= a.capIn;   // (after the K scale: the cap is on the score the softmax would see)
  const float vscale = a.valueScale ? a.valueScale[kvh] : 1.0f;

  // ---- the lane's packed row
  const uint32_t M = a.G * RB;
  const uint32_t p = (uint32_t)wave * 32u + (uint32_t)q, pc = min(p, M - 1);
  const uint32_t qhead = kvh * a.G + pc / RB, rowt = r0 + pc % RB;
  const bool live = p < M && rowt < qn;
  const uint32_t row = min(rowt, qn - 1);   // (rows at or past qn are not read: the lane repeats the last live one)
  v8 qf[NKS];
  {
    const int64_t qseq = RAGGED ? (int64_t)packed * a.ldq : (int64_t)batch * a.bsq;
    const char *qp = a.q + (qseq + (int64_t)qhead * a.hsq + (int64_t)row * a.ldq) * 2;
#pragma unroll
    for (int s = 0; s < NKS; ++s) qf[s] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (16 * s + 8 * hi) * 2));
  }
  // keys this row sees
  // (TREE: the row's mask, cut to the live nodes -- with n < qn keys the rows from n on have no key of their own)
  const auto keys = [&]() MFA_PREFILL_INLINE {
    if constexpr (TREE) {
      const uint32_t liveNodes = min(qn, n);
      const uint64_t word = a.masks[(int64_t)batch * a.maskStride + row];
      const uint64_t mask = liveNodes < 64u ? word & ((1ull << liveNodes) - 1ull) : word;
      return VisibleKeys<true, true, false, 64>(n, TreeRow{n > qn ? n - qn : 0u, mask}, a.window, a.sinkTokens);
    } else {
      return VisibleKeys<WINDOW, SINK, CAP>(n, row + (n > qn ? n - qn : 0u) + 1u, a.causal, a.window, a.sinkTokens);
    }
  }();

  // ---- addresses of a 16-key group (wave-uniform; element offsets from a.k / a.v)
  const int64_t ldk = a.ldk, ldv = a.ldv, psk = a.psk, psv = a.psv;   // (values, not fields of `a`: hipcc otherwise selects between
  const bool paged = a.paged != 0;                                     //  the FIELDS' addresses and parks the block in scratch)
  const int64_t khead = (int64_t)kvh * a.hsk, vhead = (int64_t)kvh * a.hsv;
  const int64_t kseq = (int64_t)batch * a.bsk + khead, vseq = (int64_t)batch * a.bsv + vhead;
  const int64_t tableRow = (int64_t)batch * a.tableStride;
  const uint32_t pageShift = a.pageShift, pageMask = (1u << pageShift) - 1u;
  auto group_offsets = [&](uint32_t key, int64_t &ko, int64_t &vo) MFA_PREFILL_INLINE {
    if (paged) {
      // (entries past the sequence's last page are never read)
      const int64_t page = key < n ? (int64_t)a.table[tableRow + (key >> pageShift)] : 0;
      const int64_t in = (int64_t)(key & pageMask);
      ko = page * psk + khead + in * ldk;
      vo = page * psv + vhead + in * ldv;
    } else {
      ko = kseq + (int64_t)key * ldk;
      vo = vseq + (int64_t)key * ldv;
    }
  };

  // ---- staging: instruction i of the workgroup covers rows i RPI .. + RPI - 1 of the tile whole; thread = (row lrow0, chunk lc).
  // The rows of one wave-instruction lie inside one 16-key group (64 / CPR consecutive rows, aligned, and 64 / CPR divides 16), so its
  // group is wave-uniform.  A thread's chunk does not depend on i.  Its row inside the group, (i RPI + lrow0) & 15, does not either
  // when an instruction covers whole groups (RPI % 16 == 0: D <= 128, and e4m3 at D = 256); a 16-bit cache at D = 256 has RPI = 8,
  // lrow0 < 8, and the row is lrow0 + (i RPI & 15): `kstep` / `vstep`, the bytes of RPI rows, are added for odd i.
  static_assert(16 % (64 / CPR) == 0 && (RPI % 16 == 0 || 16 % RPI == 0),
                "the rows of a wave-instruction stay inside a 16-key group, and those of a workgroup-instruction tile the groups");
  u32x4 kreg[NCH], vreg[NCH];
  const int lrow0 = tid / CPR, lc = tid % CPR;
  const int64_t kin = (int64_t)(lrow0 & 15) * ldk * ESZ + lc * 16, vin = (int64_t)(lrow0 & 15) * ldv * ESZ + lc * 16;   // bytes
  const int64_t kstep = (int64_t)RPI * ldk * ESZ, vstep = (int64_t)RPI * ldv * ESZ;   // (RPI < 16 only)
  auto issue_loads = [&](uint32_t key0) MFA_PREFILL_INLINE {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int r = j * RPI + lrow0;
      const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane(r >> 4);
      int64_t ko, vo;
      group_offsets(key0 + 16u * g, ko, vo);
      u32x4 zk = {0u, 0u, 0u, 0u}, zv = {0u, 0u, 0u, 0u};
      if (key0 + (uint32_t)r < n) {   // rows at or past n are never loaded: zeros
        if constexpr (RPI % 16 == 0) {
          zk = *reinterpret_cast<const u32x4 *>(a.k + ko * ESZ + kin);
          zv = *reinterpret_cast<const u32x4 *>(a.v + vo * ESZ + vin);
        } else {
          const int into = (j * RPI & 15) / RPI;   // whole instructions into the group: a constant of the unrolled loop
          zk = *reinterpret_cast<const u32x4 *>(a.k + ko * ESZ + kin + into * kstep);
          zv = *reinterpret_cast<const u32x4 *>(a.v + vo * ESZ + vin + into * vstep);
        }
      }
      kreg[j] = zk;
      vreg[j] = zv;
    }
  };
  // 16-bit chunk c (8 values of d) of key row r: K image row-major, chunk kswz(r, c); V image [D/32][64 keys][32 d]
  auto write_lds = [&](int buf) MFA_PREFILL_INLINE {
    char *Ks = smem + buf * STAGE, *Vs = Ks + KIMG;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int r = j * RPI + lrow0;
      if constexpr (FP8) {
        const int c = 2 * lc;
        *reinterpret_cast<u32x4 *>(Ks + r * ROWB + kswz<D>(r, c) * 16) = cvt8_e4m3<T>(kreg[j][0], kreg[j][1]);
        *reinterpret_cast<u32x4 *>(Ks + r * ROWB + kswz<D>(r, c + 1) * 16) = cvt8_e4m3<T>(kreg[j][2], kreg[j][3]);
        char *dst = Vs + ((c >> 2) * PF_TILE + r) * 64 + (c & 3) * 16;
        *reinterpret_cast<u32x4 *>(dst) = cvt8_e4m3<T>(vreg[j][0], vreg[j][1]);
        *reinterpret_cast<u32x4 *>(dst + 16) = cvt8_e4m3<T>(vreg[j][2], vreg[j][3]);
      } else {
        *reinterpret_cast<u32x4 *>(Ks + r * ROWB + kswz<D>(r, lc) * 16) = kreg[j];
        *reinterpret_cast<u32x4 *>(Vs + ((lc >> 2) * PF_TILE + r) * 64 + (lc & 3) * 16) = vreg[j];
      }
    }
  };

  f32x16 o[NDB];
  float m = STEP_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  const int vtr_off = vtr_lane_offset(lane, hi);

  // A fragment t of key row kr = 32 half + q: chunk kswz(kr, 2 t + hi).  The swizzle XORs the chunk with bits of the row that 32 half
  // does not touch, 2 t + hi = 2 t ^ hi, and a row starts on a multiple of its own size (a power of two): the byte offset is
  // (offset of t = 0, half = 0) ^ 32 t, plus 32 half rows -- one register and immediates.
  static_assert((ROWB & (ROWB - 1)) == 0, "a K image row is a power of two");
  const int kfrag0 = q * ROWB + kswz<D>(q, hi) * 16;

  // step `half` (32 keys) of a tile from the images of `buf`; MASK = the per-element mask (tiles at or past first_masked)
  auto compute = [&](auto maskTag, uint32_t key0, int buf, int half) MFA_PREFILL_INLINE {
    constexpr bool MASK = decltype(maskTag)::value;
    const char *Ks = smem + buf * STAGE, *Vs = Ks + KIMG;
    {
      const uint32_t cur = key0 + 32u * half;
      // ---- S^T = K Q^T: s[r] = key cur + crow(r, hi), packed row q
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
      for (int t = 0; t < NKS; ++t) {
        const u32x4 kf = *reinterpret_cast<const u32x4 *>(Ks + 32 * half * ROWB + (kfrag0 ^ (32 * t)));
        s = F::mfma(__builtin_bit_cast(v8, kf), qf[t], s);
      }
      // ---- online softmax over the visible keys only (the K scale rides on the softmax scale)
      if constexpr (CAP) rescale_row(score_max<MASK, true>(s, keys, cur, hi, kscale, a.capOut), m, l, o);
      else rescale_row(score_max<MASK>(s, keys, cur, hi, kscale), m, l, o);
      v8 pf[2];
      l += score_exp<T, MASK>(s, keys, cur, hi, m, pf);
      // ---- O^T += V^T P^T
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * PF_TILE + 32 * half + 16 * u) * 64 + vtr_off, pf[u], o[db]);
    }
  };

  // ---- the tiles: the loads of tile t + 1 fly under the arithmetic of tile t and land in the other buffer behind it.  One barrier
  // per tile: the buffer written in iteration t was last read in iteration t - 1, which every wave left through that barrier.
  if constexpr (SPLIT) {   // (the piece's first tile)
    if (sinkEnd > sinkBegin || endTile > beginTile) {
      issue_loads((sinkEnd > sinkBegin ? sinkBegin : beginTile) * PF_TILE);
      write_lds(0);
    }
  } else if constexpr (SINK) {
    if (sinkEnd != 0 || endTile > beginTile) {
      issue_loads((sinkEnd ? 0u : beginTile) * PF_TILE);
      write_lds(0);
    }
  } else if (endTile > beginTile) {
    issue_loads(beginTile * PF_TILE);
    write_lds(0);
  }
  __syncthreads();
  // (sinkZone: a tile of [0, sinkEnd); the tile walked after the last of them is beginTile, and a buffer is a position in the list)
  auto tile = [&](auto maskTag, auto sinkZone, uint32_t t) MFA_PREFILL_INLINE {
    bool more = t + 1 < endTile;
    uint32_t next = t + 1;
    int buf = (int)((t - beginTile) & 1u);
    if constexpr (SINK) {
      if constexpr (decltype(sinkZone)::value) {
        more = t + 1 < sinkEnd || endTile > beginTile;
        next = t + 1 < sinkEnd ? t + 1 : beginTile;
        buf = (int)((SPLIT ? t - sinkBegin : t) & 1u);   // (SPLIT: a buffer is a position inside the piece)
      } else {
        buf = (int)((t - beginTile + (SPLIT ? sinkEnd - sinkBegin : sinkEnd)) & 1u);
      }
    }
    if (more) issue_loads(next * PF_TILE);
    compute(maskTag, t * PF_TILE, buf, 0);
    compute(maskTag, t * PF_TILE, buf, 1);
    if (more) write_lds(buf ^ 1);
    __syncthreads();
  };
  // (two loops, not one loop with the choice inside: with both forms of a step merging in one loop body hipcc spilled 6 .. 19 VGPRs
  // of the D = 128 kernels; like this the largest takes 232 of 256)
  if constexpr (SINK)     // (a fourth loop ahead of them all: the sink tiles)
    for (uint32_t ts = SPLIT ? sinkBegin : 0u; ts < sinkEnd; ++ts) tile(std::true_type{}, std::true_type{}, ts);
  uint32_t t = beginTile;
  if constexpr (WINDOW)   // (a third loop in front: the tiles in which some row's window starts)
    for (; t < unmaskedBegin; ++t) tile(std::true_type{}, std::false_type{}, t);
  for (; t < firstMasked; ++t) tile(std::false_type{}, std::false_type{}, t);
  for (; t < endTile; ++t) tile(std::true_type{}, std::false_type{}, t);

  // ---- normalise and store straight from the accumulators: o[db][4 g + i] is d = 32 db + 8 g + 4 hi + i of the lane's row
  float l_tot = l + __shfl_xor(l, 32);
  if (!live) return;
  if constexpr (SPLIT) {
    // the piece's slab: (m, l) always, O where the row saw a key (the combine kernel reads O only where l > 0); no scale, no sink logit
    const uint64_t slab = (((uint64_t)(blockIdx.x % a.pieces) * a.batches + batch) * a.heads + qhead) * a.rows + rowt;
    if (hi == 0) *reinterpret_cast<float2 *>(a.wsML + slab * 2) = make_float2(m, l_tot);
    if (l_tot > 0.f) {
      float *dst = a.wsO + slab * D + 4 * hi;
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4 *>(dst + 32 * db + 8 * g) = make_float4(o[db][4 * g], o[db][4 * g + 1], o[db][4 * g + 2], o[db][4 * g + 3]);
    }
    return;
  }
  // SINK: the sink logit joins (m, l); `fold` rescales O with l.  A row without a visible key ends with m = s2, l = 1
  float fold = 1.0f;
  if constexpr (SINK) {
    if (a.sinkLogits) fold = fold_sink_logit<CAP>(a.sinkLogits[qhead], m, l_tot);
  }
  const float inv = l_tot > 0.f ? vscale * fold / l_tot : 0.f;   // a row without a visible key: O = 0
  const int64_t at = (RAGGED ? (int64_t)packed * a.ldo : (int64_t)batch * a.bso) + (int64_t)qhead * a.hso + (int64_t)rowt * a.ldo;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 x = make_float4(o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
      store_o4<T>(a.o, at + 32 * db + 8 * g + 4 * hi, a.outF32, x);
    }
  if (hi == 0 && a.l) a.l[(RAGGED ? (int64_t)packed : (int64_t)batch * a.lbs) + (int64_t)qhead * a.lhs + rowt] = row_lse(m, l_tot);
}

// SPLIT: merges the pieces of a row (the online-softmax merge of decode16_combine_body, attn_decode16.h).  One wave per (sequence, head,
// row) of the capacity: lane s holds (m_s, l_s) of piece s (pieces <= 64); for O the wave is D / 4 column lanes x 64 / (D / 4) piece
// groups.  A piece's weight is exp2(m_s - m*) where its l > 0 and 0 elsewhere, and its O slab is read only where the weight is not 0:
// nothing is read that the launch did not write.  Rows at or past queryLengths[b] are skipped whole.  The sink logit joins the merged
// (m*, l*) and the value scale the normalisation, HERE and nowhere else: once per row.  A row without a visible key in any piece:
// O = 0, L = -FLT_MAX or the sink logit.
template <typename T, int D>
__device__ __forceinline__ void prefill16_combine_body(const PrefillArgs &a) {
  const int lane = threadIdx.x & 63;
  const uint32_t R = a.rows, S = a.pieces;
  const uint64_t rows = (uint64_t)a.batches * a.heads * R;
  const uint64_t rowid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rowid >= rows) return;
  const uint32_t row = (uint32_t)(rowid % R), bh = (uint32_t)(rowid / R);
  const uint32_t head = bh % a.heads, batch = bh / a.heads;
  const uint32_t qn = a.qlengths ? min(a.qlengths[batch], R) : R;
  if (row >= qn) return;   // (its slabs were never written)
  float ms = STEP_MINUS_HUGE, ls = 0.f;
  if ((uint32_t)lane < S) {
    const float2 ml = *reinterpret_cast<const float2 *>(a.wsML + ((uint64_t)lane * rows + rowid) * 2);
    ms = ml.x; ls = ml.y;
  }
  float mstar = ms;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mstar = fmaxf(mstar, __shfl_xor(mstar, off, 64));
  const float w = ((uint32_t)lane < S && ls > 0.f) ? fast_exp2(ms - mstar) : 0.f;
  float lstar = w * ls;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) lstar += __shfl_xor(lstar, off, 64);
  constexpr uint32_t CL = D / 4, GR = 64 / CL;
  const uint32_t c = (uint32_t)lane % CL, g = (uint32_t)lane / CL;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (uint32_t s0 = 0; s0 < S; s0 += GR) {
    const uint32_t s_ = s0 + g;
    const float ws = __shfl(w, (int)(s_ < 64 ? s_ : 63), 64);   // (every lane takes part in the exchange)
    if (s_ < S && ws > 0.f) {
      const float4 x = *reinterpret_cast<const float4 *>(a.wsO + ((uint64_t)s_ * rows + rowid) * D + c * 4);
      acc.x += ws * x.x; acc.y += ws * x.y; acc.z += ws * x.z; acc.w += ws * x.w;
    }
  }
#pragma unroll
  for (uint32_t off = CL; off < 64; off <<= 1) {
    acc.x += __shfl_xor(acc.x, (int)off, 64); acc.y += __shfl_xor(acc.y, (int)off, 64);
    acc.z += __shfl_xor(acc.z, (int)off, 64); acc.w += __shfl_xor(acc.w, (int)off, 64);
  }
  float fold = 1.0f;
  if (a.sinkLogits) fold = fold_sink_logit(a.sinkLogits[head], mstar, lstar);
  const float vscale = a.valueScale ? a.valueScale[head / a.G] : 1.0f;
  const float inv = lstar > 0.f ? vscale * fold / lstar : 0.f;
  if (g == 0) {
    acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
    const int64_t at = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)row * a.ldo + 4 * c;
    store_o4<T>(a.o, at, a.outF32, acc);
  }
  if (lane == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + row] = row_lse(mstar, lstar);
}

} // namespace mfa

// One list of the kernel families, (infix, WINDOW, SINK, RAGGED, CAP, TREE, SPLIT): the kernels, the table that selects them (attn_prefill16.hip) and the
// names are generated from it.  MFA_PREFILL_KERNELS(MFA_PREFILL_DEFINE, ...) is a set's code objects, in the translation unit that
// holds them; (MFA_PREFILL_DECLARE, ...) names the kernels of another unit for the table.  D = 256 runs one workgroup per compute unit.
#define MFA_PREFILL_FAMILIES(X, K, TN, T, D)                                                                                          \
  X(K, , false, false, false, false, false, false, TN, T, D) X(K, w, true, false, false, false, false, false, TN, T, D)               \
  X(K, s, true, true, false, false, false, false, TN, T, D) X(K, r, true, true, true, false, false, false, TN, T, D)                  \
  X(K, c, true, true, false, true, false, false, TN, T, D) X(K, rc, true, true, true, true, false, false, TN, T, D)                   \
  X(K, t, true, true, false, false, true, false, TN, T, D) X(K, sk, true, true, false, false, false, true, TN, T, D)                  \
  X(K, tk, true, true, false, false, true, true, TN, T, D)
#define MFA_PREFILL_DEFINE(NAME, D, ...)                                                                                              \
  extern "C" __global__ __launch_bounds__(256, D == 256 ? 1 : 2) void NAME(const mfa::PrefillArgs a) { mfa::prefill16_body<__VA_ARGS__>(a); }
#define MFA_PREFILL_DECLARE(NAME, D, ...) extern "C" __global__ void NAME(const mfa::PrefillArgs a);
#define MFA_PREFILL_FAMILY(K, I, WINDOW, SINK, RAGGED, CAP, TREE, SPLIT, TN, T, D)                                                    \
  K(attn_prefill16##I##_d##D##_##TN, D, T, D, false, WINDOW, SINK, RAGGED, CAP, TREE, SPLIT)                                          \
  K(attn_prefill16##I##_d##D##_##TN##_e4m3, D, T, D, true, WINDOW, SINK, RAGGED, CAP, TREE, SPLIT)
#define MFA_PREFILL_KERNELS(K, TN, T, D) MFA_PREFILL_FAMILIES(MFA_PREFILL_FAMILY, K, TN, T, D)
// the combine kernel of a (D, type), in the translation unit of the set: the e4m3 launches share it (the slabs hold FP32 whatever the cache)
#define MFA_PREFILL_COMBINE_DEFINE(TN, T, D)                                                                                          \
  extern "C" __global__ __launch_bounds__(256) void attn_prefill16_combine_d##D##_##TN(const mfa::PrefillArgs a) {                    \
    mfa::prefill16_combine_body<T, D>(a);                                                                                             \
  }
#define MFA_PREFILL_COMBINE_DECLARE(TN, T, D) extern "C" __global__ void attn_prefill16_combine_d##D##_##TN(const mfa::PrefillArgs a);
