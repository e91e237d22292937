// attn_decode16.h -- decode attention on the 16-bit matrix cores of gfx950: R new query rows per sequence against a long cache of
// keys and values (include/mfa_decode.h; an extension of this port).
//
// The work is bound by the bytes of K and V, so the kernel is built around reading them once and keeping many loads in flight:
//   * one workgroup (4 waves) serves ONE K / V head of one sequence (and one piece of its keys): the G query heads x R rows that share
//     the head are packed as the M = G R <= 32 columns of one 32-wide matrix tile, so K and V are read once, not G times.
//   * every wave walks its own 32-key steps (wave w takes steps w, w + 4, ... of the piece) with its own running (m, l, O): no barrier
//     inside the loop.  The four partial results are merged through LDS once, at the end.
//   * S^T = K Q^T with v_mfma_f32_32x32x16 (the fragment maps of dev/attn_fwd16.h: a lane owns one packed query row, softmax is
//     lane-local plus one half-wave exchange).  K goes from memory STRAIGHT to registers as the A operand (a lane = a key row, 16-byte
//     loads); V is loaded as whole rows (coalesced), written to a wave-private LDS image [D/32][32 keys][32 d] and gathered as V^T by
//     ds_read_b64_tr_b16.  The loads of the wave's next step are issued as soon as the registers of the current one are consumed.
//   * keys are addressed in groups of 16 (a tile starts on a multiple of 64 and a page holds at least 16 keys, so a group never
//     straddles a page): two wave-uniform block-table reads per step, none per lane.
//   * what may hold poison is never loaded: key rows at or past the piece's end come in as zeros (K and V), a masked score is REPLACED
//     (p = 0 exactly), and the running maximum only ever sees visible keys -- a step, a wave or a piece without a visible key keeps
//     m = -FLT_MAX, l = 0.
//   * SPLIT: piece p of sequence b takes decode_piece_range(len_b, pieces, p) -- the same function the host exports -- and publishes
//     un-normalised O, m, l in FP32 (wsO [pieces][B Hq R][D], wsML [pieces][B Hq R][2]); attn_decode16_combine merges them.
//   * D = 256: one workgroup per compute unit.  Over a 16-bit cache O^T, a step's K and V and the Q fragments do not
//     fit the registers together: the Q fragments are parked once in LDS behind the four V images and re-read at their matrix
//     instruction (QLDS below).  The e4m3 kernels, whose K and V take half the registers, keep them in registers as at every width.
//
// FP8: the same body over an FP8 (OCP e4m3) KV cache (include/mfa_kvcache.h), K and V read as bytes.  Everything above
// holds, and so do decode_piece_range, the workspace slabs and the combine kernel.  What the parameter switches:
//   * Q stays 16-bit; K and V bytes are CONVERTED in registers to the launch's 16-bit type (cvt8_e4m3, kv_e4m3.h: exact) and feed the
//     same v_mfma_f32_32x32x16.  The FP8 matrix instruction is not used: the kernel is bound by bytes, not by the matrix pipe.
//   * K: a lane is still a key row, but a 16-byte load now spans 16 values of d.  The loads stay 16 bytes wide (half as many per step)
//     and the contraction index is permuted instead: matrix step 2u + v of the lane half `hi` contracts d = 32 u + 16 hi + 8 v .. + 7,
//     the bytes 8 v .. 8 v + 7 of load u, and the Q fragments are loaded with the same permutation.  The raw bytes wait in registers;
//     a slice is converted at its matrix instruction.
//   * V: 16-byte loads of whole rows (half as many per step), converted before the LDS write, so that the wave's V image
//     [D/32][32 keys][32 d] and the ds_read_b64_tr_b16 gather are those of the 16-bit kernel.
//   * the scales are per K / V head: keyScale folds into the softmax scale, valueScale into the final normalisation (pieces: into
//     the un-normalised O they publish, so that the combine kernel needs no change).  The 16-bit kernels read neither.
//   * poison: rows at or past the piece's end are not loaded (zero bytes = +0.0), so a 0x7f beyond a length never reaches a product.
//
// WINDOW, SINK: the rule of which keys a row sees, and the sink logit, are attn_cache_step.h's.  What is decode's own:
//   * WINDOW: the keys the workgroup walks come from decode_window_piece_range, in the unsplit kernel too (one piece of one): they
//     start at the tile of row 0's first key, and nothing below it is loaded -- no key, no page, no block-table entry (group_offsets
//     is only ever asked for keys at or past `begin`).  Pieces may be empty: they publish m = -FLT_MAX, l = 0 and zeros, which the
//     combine kernel already weighs with 0.  With W >= column + rows the ranges are decode_piece_range's.
//   * SINK tokens: the workgroup walks a piece of the tile LIST [0, sinkTiles) ++ [first, last) (decode_sink_piece_range): at most two
//     key ranges.  The loop runs over the list's own key positions -- `key0` counts keys of the piece, sink range first -- and
//     list_key() turns a position into the cache's key where one is addressed or masked; nothing between the two ranges is loaded.
//   * SINK logit: the unsplit kernel adds it at the final normalisation; in the split kernels piece 0 folds it into the (m, l) it
//     publishes -- an empty piece 0 publishes m = s2, l = 1, O = 0 -- so the combine kernel is reused as it stands.
//
// CAP: the soft cap of attn_cache_step.h on the visible scores, the SINK body otherwise (any window and sinks, none included): c1 rides
// on kscale, c2 goes to score_max.  Pieces, workspace and the combine kernel are untouched -- the pieces publish capped (m, l).
//
// TREE: the tree rule of attn_cache_step.h, the SINK body otherwise (any window and sinks, none included).  The lane's mask is that of
// its ROW, pc % R, never of its packed index; R <= 32, so the low word of the uint64 is all a lane keeps.  Nothing else moves: row 0's
// frontier P + 1 is the smallest a node can have, so decode_sink_piece_range with `rows` already starts at the conservative tile, and
// the pieces, the workspace and the combine kernel are the sink launch's.
#pragma once
#include "attn_cache_step.h"
#include "kv_e4m3.h"

namespace mfa {

constexpr int DEC_KEY_TILE = 64;   // pieces are whole tiles of this many keys (MFA_DECODE_KEY_TILE)
constexpr int DEC_STEP = 32;       // keys per wave step
constexpr int DEC_WAVES = 4;

struct DecodeArgs {
  const char *q, *k, *v;
  char *o;
  float *l;                       // null: not stored
  const uint32_t *lengths;
  const int32_t *table;           // paged launches
  int64_t tableStride;
  int64_t ldq, hsq, bsq;          // elements
  int64_t ldk, hsk, bsk, psk;     // (K, V of an e4m3 cache: an element is a byte)
  int64_t ldv, hsv, bsv, psv;
  int64_t ldo, hso, bso;
  int64_t lhs, lbs;
  uint32_t R, G, Hq, Hkv, batches, column;
  uint32_t paged, pageShift;      // pageSize = 1 << pageShift
  uint32_t causal, outF32;
  uint32_t pieces;
  float scale2;                   // log2(e) / sqrt(D)
  float *wsO, *wsML;
  const float *keyScale, *valueScale;   // e4m3 caches, per K / V head; null: 1.0
  uint32_t window;                      // the WINDOW kernels only (>= 1); last, so that no other field moves
  uint32_t sinkTokens;                  // the SINK kernels only, which also take window = 0 (no window); behind `window` in turn
  const float *sinkLogits;              // [Hq], natural units; null: none
  float capIn, capOut;                  // the CAP kernels only: c1 = 2 / cap and c2 = cap log2(e) (attn_cache_step.h); behind the sinks in turn
  const uint64_t *masks;                // the TREE kernels only: [batches][R] row masks (include/mfa_tree.h); last in turn
  int64_t maskStride;                   // elements between two sequences' masks; 0: one tree for all
};

// The two key ranges of piece `piece` of `pieces` with `sinkTokens` sink keys under a window of `window` keys (0: no window, lo0 = 0):
// with lo0 the first key row 0 sees, first = lo0 / 64, last = ceil(length / 64) -- [first, last) are the tiles that hold a key some row
// sees through its window -- and sinkTiles = min(ceil(min(S, length) / 64), first), an equal share, in whole 64-key tiles, of the LIST
// [0, sinkTiles) ++ [first, last): [begin[0], end[0]) inside the sink tiles, [begin[1], end[1]) inside the window's; only the last tile
// of the sequence may be partial.  Device and host (mfa_attention_decode_sink_piece_range) run this one body.
__host__ __device__ __forceinline__ void decode_sink_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t sinkTokens,
                                                                 uint32_t pieces, uint32_t piece, uint32_t *begin, uint32_t *end) {
  const uint64_t f1 = (length > rows ? (uint64_t)length - rows : 0) + 1;   // row 0's frontier + 1
  const uint64_t lo0 = window ? window_lo<uint64_t>(f1, window) : 0;
  const uint64_t first = lo0 / DEC_KEY_TILE, last = ((uint64_t)length + DEC_KEY_TILE - 1) / DEC_KEY_TILE;
  const uint64_t sunk = sinkTokens < length ? sinkTokens : length;
  uint64_t sinkTiles = (sunk + DEC_KEY_TILE - 1) / DEC_KEY_TILE;
  if (sinkTiles > first) sinkTiles = first;
  const uint64_t tiles = sinkTiles + (last > first ? last - first : 0);
  const uint64_t t0 = (uint64_t)piece * tiles / pieces, t1 = ((uint64_t)piece + 1) * tiles / pieces;   // positions in the list
  const uint64_t tb[2] = {t0 < sinkTiles ? t0 : sinkTiles, first + (t0 > sinkTiles ? t0 - sinkTiles : 0)};
  const uint64_t te[2] = {t1 < sinkTiles ? t1 : sinkTiles, first + (t1 > sinkTiles ? t1 - sinkTiles : 0)};
  for (int i = 0; i < 2; ++i) {
    uint64_t b = tb[i] * DEC_KEY_TILE, e = te[i] * DEC_KEY_TILE;
    if (e > length) e = length;
    if (b > e) b = e;
    begin[i] = (uint32_t)b;
    end[i] = (uint32_t)e;
  }
}

// keys [*begin, *end) of a piece under a window of `window` >= 1 keys and no sink tokens: the list is [first, last) alone
// (mfa_attention_decode_window_piece_range)
__host__ __device__ __forceinline__ void decode_window_piece_range(uint32_t length, uint32_t rows, uint32_t window, uint32_t pieces,
                                                                   uint32_t piece, uint32_t *begin, uint32_t *end) {
  uint32_t b[2], e[2];
  decode_sink_piece_range(length, rows, window, 0, pieces, piece, b, e);
  *begin = b[1];
  *end = e[1];
}

// keys [*begin, *end) of a piece without a window: an equal share of all the sequence's tiles (mfa_attention_decode_piece_range)
__host__ __device__ __forceinline__ void decode_piece_range(uint32_t length, uint32_t pieces, uint32_t piece, uint32_t *begin,
                                                            uint32_t *end) {
  uint32_t b[2], e[2];
  decode_sink_piece_range(length, 1, 0, 0, pieces, piece, b, e);
  *begin = b[1];
  *end = e[1];
}

template <int D> constexpr int decode16_lds_bytes() {
  constexpr int images = DEC_WAVES * DEC_STEP * D * 2;
  constexpr int merge = DEC_WAVES * 32 * (D + 4) * 4 + 2 * DEC_WAVES * 32 * 4;
  return images > merge ? images : merge;
}

template <typename T, int D, bool SPLIT, bool FP8, bool WINDOW = false, bool SINK = false, bool CAP = false, bool TREE = false>
__device__ __forceinline__ void decode_body(const DecodeArgs &a) {
  static_assert(!CAP || SINK, "the capped kernels are the sink kernels plus CAP");
  static_assert(!TREE || (SINK && !CAP), "the tree kernels are the sink kernels plus TREE");
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ESZ = FP8 ? 1 : 2;             // bytes of a cache element
  constexpr int NDB = D / 32, NKS = D / 16;    // matrix steps along d
  constexpr int NKL = D * ESZ / 32;            // 16-byte K loads per lane
  constexpr int CPR = D * ESZ / 16;            // 16-byte chunks per row
  constexpr int RPI = 64 / CPR;                // V rows one wave-instruction covers
  constexpr int NCH = DEC_STEP / RPI;          // V chunks per lane per step
  constexpr int IMAGE = DEC_STEP * D * 2;      // bytes of a wave's V image (16-bit values)
  static_assert(16 % RPI == 0, "a lane's V rows of one instruction stay inside a 16-key group");
  // D = 256 over a 16-bit cache: K, V and O alone fill the registers, so the Q fragments are parked in LDS behind the four V images
  // and re-read at their matrix instruction.  Everything else holds them in registers.
  constexpr bool QLDS = D == 256 && !FP8;
  constexpr int QPARK = DEC_WAVES * IMAGE;     // QLDS: fragment s of lane i at QPARK + (s 64 + i) 16, the same for every wave
  static_assert(!QLDS || QPARK + NKS * 64 * 16 <= decode16_lds_bytes<D>(), "the parked Q fragments fit the workgroup's LDS");

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, q = lane & 31, hi = lane >> 5;
  const uint32_t piece = SPLIT ? blockIdx.x % a.pieces : 0u;
  const uint32_t hb = SPLIT ? blockIdx.x / a.pieces : blockIdx.x;
  const uint32_t kvh = hb % a.Hkv, batch = hb / a.Hkv;
  const uint32_t R = a.R, M = a.G * R;
  const uint32_t len = min(a.lengths[batch], a.column);
  uint32_t begin = 0, end = len;
  // SINK: [begin, end) are positions in the piece's own key list -- `sunk` keys of the sink range from key sinkBegin, then the
  // window range from key windowBegin -- and list_key() is the cache's key at a position
  uint32_t sunk = 0, sinkBegin = 0, windowBegin = 0;
  if constexpr (SINK) {
    uint32_t rb[2], re[2];
    decode_sink_piece_range(len, R, a.window, a.sinkTokens, SPLIT ? a.pieces : 1u, piece, rb, re);
    sunk = re[0] - rb[0]; sinkBegin = rb[0]; windowBegin = rb[1];
    end = sunk + (re[1] - rb[1]);
  } else if constexpr (WINDOW) decode_window_piece_range(len, R, a.window, SPLIT ? a.pieces : 1u, piece, &begin, &end);
  else if constexpr (SPLIT) decode_piece_range(len, a.pieces, piece, &begin, &end);
  auto list_key = [&](uint32_t at) { return SINK ? (at < sunk ? sinkBegin + at : windowBegin + (at - sunk)) : at; };
  const uint32_t tableEnd = SINK ? len : end;   // block-table entries are read for keys below it
  float kscale = a.scale2, vscale = 1.0f;   // (16-bit: scale2 as it stands, and vscale is never used)
  if constexpr (FP8) {
    kscale = a.scale2 * (a.keyScale ? a.keyScale[kvh] : 1.0f);
    vscale = a.valueScale ? a.valueScale[kvh] : 1.0f;
  }
  if constexpr (CAP) kscale *= a.capIn;   // (after the K scale: the cap is on the score the softmax would see)

  // ---- the lane's packed query row: p = (query head within the group) R + row; columns >= M repeat the last one and are not stored
  // (FP8: its fragments in the permuted contraction order of the K bytes)
  const uint32_t pc = min((uint32_t)q, M - 1);
  const uint32_t qhead = kvh * a.G + pc / R, qrow = pc % R;
  v8 qf[QLDS ? 1 : NKS];
  const char *qpark = smem + QPARK + lane * 16;
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)qhead * a.hsq + (int64_t)qrow * a.ldq) * 2;
    if constexpr (QLDS) {   // wave w parks the fragments w, w + 4, ...: a lane's fragments do not depend on its wave
      for (int s = wave; s < NKS; s += DEC_WAVES)
        *reinterpret_cast<u32x4 *>(smem + QPARK + (s * 64 + lane) * 16) = *reinterpret_cast<const u32x4 *>(qp + (16 * s + 8 * hi) * 2);
      __syncthreads();
    } else {
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        const int d0 = FP8 ? 32 * (s >> 1) + 16 * hi + 8 * (s & 1) : 16 * s + 8 * hi;
        qf[s] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + d0 * 2));
      }
    }
  }
  // keys this row sees (causal: c <= row + max(len - R, 0); always c < len, and inside this piece c < end)
  // (TREE: the row's mask, cut to the live nodes -- with len < R new tokens the rows from `len` on have no key of their own)
  const auto keys = [&] {
    if constexpr (TREE) {
      const uint32_t live = min(R, len);
      const uint32_t word = *reinterpret_cast<const uint32_t *>(a.masks + ((int64_t)batch * a.maskStride + qrow));   // the low word
      const uint32_t mask = live < 32u ? word & ((1u << live) - 1u) : word;
      return VisibleKeys<true, true, false, 32>(len, TreeRow{len > R ? len - R : 0u, mask}, a.window, a.sinkTokens);
    } else {
      return VisibleKeys<WINDOW, SINK, CAP>(SINK ? len : end, qrow + (len > R ? len - R : 0u) + 1u, a.causal, a.window, a.sinkTokens);
    }
  }();

  // ---- addresses of a step's two 16-key groups (wave-uniform; element offsets from a.k / a.v, which are byte offsets under FP8)
  const int64_t khead = (int64_t)kvh * a.hsk, vhead = (int64_t)kvh * a.hsv;
  const uint32_t pageMask = (1u << a.pageShift) - 1u;
  auto group_offsets = [&](uint32_t key0, int64_t (&ko)[2], int64_t (&vo)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t key = key0 + 16u * u;
      if (a.paged) {
        // (entries past the sequence's last page are never read)
        const int64_t page = key < tableEnd ? (int64_t)a.table[(int64_t)batch * a.tableStride + (key >> a.pageShift)] : 0;
        const int64_t in = (int64_t)(key & pageMask);
        ko[u] = page * a.psk + khead + in * a.ldk;
        vo[u] = page * a.psv + vhead + in * a.ldv;
      } else {
        ko[u] = (int64_t)batch * a.bsk + khead + (int64_t)key * a.ldk;
        vo[u] = (int64_t)batch * a.bsv + vhead + (int64_t)key * a.ldv;
      }
    }
  };

  // K: lane = key row q of the step, chunks 2t + hi (the A operand as it stands; FP8: bytes 32 t + 16 hi .. + 15 of the row).
  // V: instruction i covers rows i RPI .. + RPI - 1 whole.
  u32x4 kreg[NKL], vreg[NCH];
  const int vrow0 = lane / CPR, vc = lane % CPR;
  auto issue_loads = [&](uint32_t key0) {
    int64_t ko[2], vo[2];
    group_offsets(list_key(key0), ko, vo);
    const bool kvalid = key0 + (uint32_t)q < end;
    const char *kp;
    if constexpr (FP8) kp = a.k + (q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk + 16 * hi;
    else kp = a.k + ((q >> 4 ? ko[1] : ko[0]) + (int64_t)(q & 15) * a.ldk + 8 * hi) * 2;
#pragma unroll
    for (int t = 0; t < NKL; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + 32 * t);
      kreg[t] = z;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = i * RPI + vrow0;
      u32x4 z = {0u, 0u, 0u, 0u};
      if (key0 + (uint32_t)row < end) {
        if constexpr (FP8) z = *reinterpret_cast<const u32x4 *>(a.v + vo[(i * RPI) >> 4] + (int64_t)(row & 15) * a.ldv + vc * 16);
        else z = *reinterpret_cast<const u32x4 *>(a.v + (vo[(i * RPI) >> 4] + (int64_t)(row & 15) * a.ldv + vc * 8) * 2);
      }
      vreg[i] = z;
    }
  };

  f32x16 o[NDB];
  float m = STEP_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  char *Vs = smem + wave * IMAGE;   // this wave's V image: [D/32][32 keys][32 d]
  const int vtr_off = vtr_lane_offset(lane, hi);

  uint32_t key0 = begin + (uint32_t)wave * DEC_STEP;
  if (key0 < end) issue_loads(key0);
  while (key0 < end) {
    // ---- S^T = K Q^T: s[r] = key key0 + crow(r, hi), packed query row q
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NKS; ++t) {
      if constexpr (FP8) {   // a slice of K is converted at its matrix instruction
        const u32x4 kb = kreg[t >> 1];
        const u32x4 kf = (t & 1) ? cvt8_e4m3<T>(kb[2], kb[3]) : cvt8_e4m3<T>(kb[0], kb[1]);
        s = F::mfma(__builtin_bit_cast(v8, kf), qf[t], s);
      } else if constexpr (QLDS) {
        s = F::mfma(__builtin_bit_cast(v8, kreg[t]), __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qpark + t * 64 * 16)), s);
      } else {
        s = F::mfma(__builtin_bit_cast(v8, kreg[t]), qf[t], s);
      }
    }
    // ---- V rows to the wave's image (the image's previous reads were issued before these writes: one wave, in order)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int row = i * RPI + vrow0;
      if constexpr (FP8) {   // converted: a lane's 16 values of d are the 16-bit chunks 2 vc and 2 vc + 1 of its row
        char *dst = Vs + ((vc >> 1) * DEC_STEP + row) * 64 + (vc & 1) * 32;
        *reinterpret_cast<u32x4 *>(dst) = cvt8_e4m3<T>(vreg[i][0], vreg[i][1]);
        *reinterpret_cast<u32x4 *>(dst + 16) = cvt8_e4m3<T>(vreg[i][2], vreg[i][3]);
      } else {
        *reinterpret_cast<u32x4 *>(Vs + ((vc >> 2) * DEC_STEP + row) * 64 + (vc & 3) * 16) = vreg[i];
      }
    }
    // ---- the registers are free: the next step's loads fly during the rest of this one
    const uint32_t cur = list_key(key0);
    key0 += DEC_WAVES * DEC_STEP;
    if (key0 < end) issue_loads(key0);

    // ---- online softmax over the visible keys only (FP8: the K scale rides on the softmax scale)
    if constexpr (CAP) rescale_row(score_max<true, true>(s, keys, cur, hi, kscale, a.capOut), m, l, o);
    else rescale_row(score_max<true>(s, keys, cur, hi, kscale), m, l, o);
    v8 pf[2];
    l += score_exp<T, true>(s, keys, cur, hi, m, pf);

    // ---- O^T += V^T P^T
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * DEC_STEP + 16 * u) * 64 + vtr_off, pf[u], o[db]);
  }

  // ---- merge the four waves through LDS: m* = max m_w, weights exp2(m_w - m*), sums of l and O (FP8: the V scale multiplies what
  // leaves the workgroup)
  constexpr int OLD = D + 4;
  float *Om = reinterpret_cast<float *>(smem);                       // [waves][32][OLD]
  float *ms = Om + DEC_WAVES * 32 * OLD, *ls = ms + DEC_WAVES * 32;   // [waves][32] each
  const float l_tot = l + __shfl_xor(l, 32);
  __syncthreads();   // every wave is done with its image
  if (hi == 0) ms[wave * 32 + q] = m;
  __syncthreads();
  float mstar = ms[q];
#pragma unroll
  for (int w = 1; w < DEC_WAVES; ++w) mstar = fmaxf(mstar, ms[w * 32 + q]);
  const float wgt = fast_exp2(m - mstar);   // (all of them -FLT_MAX: 1, on zeros)
  {
    float *orow = Om + (wave * 32 + q) * OLD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g)   // crow(4g + i, hi) = i + 8g + 4hi
        *reinterpret_cast<float4 *>(orow + 32 * db + 8 * g + 4 * hi) =
            make_float4(o[db][4 * g] * wgt, o[db][4 * g + 1] * wgt, o[db][4 * g + 2] * wgt, o[db][4 * g + 3] * wgt);
    if (hi == 0) ls[wave * 32 + q] = l_tot * wgt;
  }
  __syncthreads();
  constexpr int CL = D / 4;   // float4 columns per row
  for (int idx = tid; idx < 32 * CL; idx += DEC_WAVES * 64) {
    const uint32_t p = (uint32_t)idx / CL, c = (uint32_t)idx % CL;
    if (p >= M) break;
    float4 acc = *reinterpret_cast<const float4 *>(Om + p * OLD + 4 * c);
    float lsum = ls[p], mrow = ms[p];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
      const float4 x = *reinterpret_cast<const float4 *>(Om + (w * 32 + p) * OLD + 4 * c);
      acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
      lsum += ls[w * 32 + p];
      mrow = fmaxf(mrow, ms[w * 32 + p]);
    }
    const uint32_t head = kvh * a.G + p / R, row = p % R;
    // SINK: the sink logit joins (m, l) -- piece 0's when the keys are split, the workgroup's otherwise; `fold` rescales O with l
    float fold = 1.0f;
    if constexpr (SINK) {
      if (a.sinkLogits && piece == 0) fold = fold_sink_logit<CAP>(a.sinkLogits[head], mrow, lsum);
    }
    if constexpr (SPLIT) {
      const size_t slab = (((size_t)piece * a.batches + batch) * a.Hq + head) * R + row;
      if constexpr (FP8) { acc.x *= vscale; acc.y *= vscale; acc.z *= vscale; acc.w *= vscale; }
      if constexpr (SINK) { acc.x *= fold; acc.y *= fold; acc.z *= fold; acc.w *= fold; }
      *reinterpret_cast<float4 *>(a.wsO + slab * D + 4 * c) = acc;
      if (c == 0) *reinterpret_cast<float2 *>(a.wsML + slab * 2) = make_float2(mrow, lsum);
    } else {
      const float inv = lsum > 0.f ? (FP8 ? vscale : 1.0f) * fold / lsum : 0.f;   // a sequence of length 0: O = 0
      acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
      const int64_t at = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)row * a.ldo + 4 * c;
      store_o4<T>(a.o, at, a.outF32, acc);
      if (c == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + row] = row_lse(mrow, lsum);
    }
  }
}

// Merge the pieces (the online-softmax merge of attn_fwd_combine, attn_fwd16_v3.h, across pieces).  One wave per query row: lane s holds
// (m_s, l_s) of piece s (pieces <= 64); for O the wave is D / 4 column lanes x 64 / (D / 4) piece groups.  A piece without keys has
// l = 0 and m = -FLT_MAX: its weight is exp2(-huge) = 0 beside any piece that saw a key, and its slab holds zeros.
template <typename T, int D>
__device__ __forceinline__ void decode16_combine_body(const DecodeArgs &a) {
  const int lane = threadIdx.x & 63;
  const uint32_t R = a.R, S = a.pieces;
  const uint64_t rows = (uint64_t)a.batches * a.Hq * R;
  const uint64_t rowid = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rowid >= rows) return;
  const uint32_t row = (uint32_t)(rowid % R), bh = (uint32_t)(rowid / R);
  const uint32_t head = bh % a.Hq, batch = bh / a.Hq;
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
  const float inv = lstar > 0.f ? 1.0f / lstar : 0.f;
  if (g == 0) {
    acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
    const int64_t at = (int64_t)batch * a.bso + (int64_t)head * a.hso + (int64_t)row * a.ldo + 4 * c;
    store_o4<T>(a.o, at, a.outF32, acc);
  }
  if (lane == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head * a.lhs + row] = row_lse(mstar, lstar);
}

} // namespace mfa

// One list of the kernel families, (infix, WINDOW, SINK, CAP, TREE): the kernels, the table that selects them (attn_decode16.hip) and the
// names are generated from it.  MFA_DECODE_KERNELS(MFA_DECODE_DEFINE, ...) is a set's code objects, in the translation unit that holds
// them; (MFA_DECODE_DECLARE, ...) names the kernels of another unit for the table.  D = 256 runs one workgroup per compute unit.
#define MFA_DECODE_FAMILIES(X, K, TN, T, D)                                                                                           \
  X(K, , false, false, false, false, TN, T, D) X(K, w, true, false, false, false, TN, T, D) X(K, s, true, true, false, false, TN, T, D) \
  X(K, c, true, true, true, false, TN, T, D) X(K, t, true, true, false, true, TN, T, D)
#define MFA_DECODE_DEFINE(NAME, BOUNDS, BODY, ...)                                                                                    \
  extern "C" __global__ BOUNDS void NAME(const mfa::DecodeArgs a) { mfa::BODY<__VA_ARGS__>(a); }
#define MFA_DECODE_DECLARE(NAME, BOUNDS, BODY, ...) extern "C" __global__ void NAME(const mfa::DecodeArgs a);
#define MFA_DECODE_FAMILY(K, I, WINDOW, SINK, CAP, TREE, TN, T, D)                                                                    \
  K(attn_decode16##I##_d##D##_##TN##_single, __launch_bounds__(256, D == 256 ? 1 : 2), decode_body, T, D, false, false, WINDOW, SINK, CAP, TREE) \
  K(attn_decode16##I##_d##D##_##TN##_pieces, __launch_bounds__(256, D == 256 ? 1 : 2), decode_body, T, D, true, false, WINDOW, SINK, CAP, TREE)  \
  K(attn_decode8##I##_d##D##_##TN##_single, __launch_bounds__(256, D == 256 ? 1 : 2), decode_body, T, D, false, true, WINDOW, SINK, CAP, TREE)   \
  K(attn_decode8##I##_d##D##_##TN##_pieces, __launch_bounds__(256, D == 256 ? 1 : 2), decode_body, T, D, true, true, WINDOW, SINK, CAP, TREE)
#define MFA_DECODE_KERNELS(K, TN, T, D)                                                                                               \
  MFA_DECODE_FAMILIES(MFA_DECODE_FAMILY, K, TN, T, D)                                                                                 \
  K(attn_decode16_d##D##_##TN##_combine, __launch_bounds__(256), decode16_combine_body, T, D)
