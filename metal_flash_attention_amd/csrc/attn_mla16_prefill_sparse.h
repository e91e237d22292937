// attn_mla16_prefill_sparse.h -- SPARSE multi-head latent attention PREFILL (include/mfa_mla_prefill_sparse.h): a block
// of new query rows per sequence, of any length, each over its own LIST of key positions, shared by all heads -- the prompt chunk of a
// model whose indexer picks the keys.  One body, mla_prefill_sparse_body<T, TILES>, that joins two designs of this directory and takes
// their pieces (constants, ListedKeys, the step header, rescale_row_uniform, vt_mfma, store_o4, row_lse) from their headers:
//
//   * the two-tile step of attn_mla16_prefill.h.  The four waves divide the 576 columns as in attn_mla16.h; a wave loads its slice of
//     the step's 32 key rows to registers (36 VGPRs) ONCE, and that one load serves TILES tiles of 32 and both products: nine matrix
//     instructions a tile against the tile's Q slice, the eight latent fragments once to the wave's V image, P V into the tile's own O^T
//     registers (64 a tile).  The partials of the tiles meet behind ONE barrier a step in exchange buffers [tile][wave][4][64] float4,
//     added in the order ((w0 + w1) + w2) + w3; the running maximum is raised behind a wave-uniform test (rescale_row_uniform).
//   * the list walk of attn_mla16_sparse.h.  Lane q of step i reads slot 32 i + q of the row's list, decides validity itself -- one
//     unsigned compare against a wave-uniform limit -- and forms its own address; a paged launch does one block-table read per lane.
//     The low word of the ballot is the step's ListedKeys mask.  The rows of step i + 1 are issued in the middle of step i, the page of
//     step i + 2 and the index of step i + 3 behind them: an address is always formed from loads issued a whole step earlier.
//   * this body's own: packing.  The rows packed into a workgroup must share one list, so a workgroup serves 32 TILES HEADS of ONE
//     (sequence, row): head = 32 TILES group + 32 tile + q, and every tile tests the SAME mask.  Grid: batches x rows x groups, group
//     fastest -- the groups of a row, which gather the same cache rows, are neighbours.  TILES = 1 is what every launch runs: the
//     sparse decode step in 64 KiB of LDS, two workgroups a compute unit.  TILES = 2 gathers a row's listed cache rows half as often
//     and was measured 1.3 x SLOWER at H = 128 (96 KiB and 491 registers leave one wave a SIMD, with nothing to run while it waits on
//     its scattered rows); it is built only with -DMFA_MLAPX_TWO_TILES, for the measurement.
//   * visibility is prefill's rule over a list: n = min(cacheLengths[b], column), qn = min(queryLengths[b], rows); slot j of row r < qn
//     is visible iff 0 <= c < n and, causal, c <= r + max(n - qn, 0).  Anything else is a hole -- -1, entries below -1 (huge unsigned
//     numbers), a position at or past n or past the frontier, the slots of a last partial step: its cache row comes in as zeros, its
//     table entry is never read, its score is replaced.  A step of 32 holes changes no bit of (m, l, O).
//   * for every row the arithmetic is mla_sparse_decode_body<T, false>'s, bit for bit: the same nine-instruction chains, the same order
//     of the partials, the same step header, the same normalisation and stores.  (A lane whose maximum does not rise multiplies by 1.0f.)
//   * what may hold poison is never loaded: a workgroup whose row is at or past qn returns ahead of every barrier and reads neither Q nor
//     the list; lanes of heads at or past H repeat the last head and store nothing; nothing past slot topk - 1 of a list is read.
//   * LDS: 4 x 8 KiB images + 2 x TILES x 16 KiB exchange buffers = 64 KiB (TILES = 1) or 96 KiB (TILES = 2).
// The walk's lambdas live in the bodies that use them: mla_sparse_decode_body keeps the code object it was measured with.
#pragma once
#include "attn_mla16_prefill.h"
#include "attn_mla16_sparse.h"

namespace mfa {

struct MlaPrefillSparseArgs {
  MlaPrefillArgs a;          // blocks = groups of heads of one (sequence, row); pieces, wsO, wsML unused
  const int32_t *indices;    // [batches][rows][topk] key positions
  int64_t irs, ibs;          // entries between the lists of two rows / two sequences
  uint32_t topk;
};

template <int TILES> constexpr int mlapx_lds() { return MLA_WAVES * MLA_IMAGE + 2 * TILES * MLA_XBUF; }

template <typename T, int TILES>
__device__ __forceinline__ void mla_prefill_sparse_body(const MlaPrefillSparseArgs &sa) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  static_assert(TILES == 1 || TILES == MLAP_TILES, "one tile (the sparse decode step) or prefill's two");
  constexpr int XBUF = TILES * MLA_XBUF;   // bytes of one exchange buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];
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

  // ---- the lane's head of each tile; heads at or past H repeat the last one and are not stored
  const int col0 = MLA_LATENT * wave + 8 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  uint32_t hp[TILES], head[TILES];
  v8 qf[TILES][MLA_NKS];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    hp[t] = (group * (uint32_t)TILES + (uint32_t)t) * MLA_ROWS + (uint32_t)q;
    head[t] = min(hp[t], H - 1);
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head[t] * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int k = 0; k < MLA_NKS; ++k)
      qf[t][k] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (k < 8 ? col0 + 16 * k : colR) * 2));
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

  // lane = the key row of slot q of the step, its slice of the row as the A operand of every tile; returns the step's mask
  u32x4 kreg[MLA_NKS];
  auto issue_loads = [&](uint32_t c, int32_t page) -> uint32_t {
    const bool kvalid = c < lim;
    const int64_t ko = a.paged ? (int64_t)page * a.psk + (int64_t)(c & pageMask) * a.ldk : (int64_t)batch * a.bsk + (int64_t)c * a.ldk;
    const char *kp = a.kv + ko * 2;
#pragma unroll
    for (int k = 0; k < MLA_NKS; ++k) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + (k < 8 ? col0 + 16 * k : colR) * 2);
      kreg[k] = z;
    }
    return (uint32_t)__ballot(kvalid);   // lanes 0 .. 31 are the step's slots
  };

  f32x16 o[TILES][MLA_NDB];
  float m[TILES], l[TILES];
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    m[t] = STEP_MINUS_HUGE;
    l[t] = 0.f;
#pragma unroll
    for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[t][db][r] = 0.f;
  }

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d], read by every tile
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  // ---- the pipeline's start: positions of the first three steps, pages of the first two, rows of the first (topk >= 1)
  uint32_t key0 = 0, buf = 0, nextBits;
  uint32_t c1, c2;   // positions of the steps after this one and after that
  int32_t page1;     // page of c1
  {
    const uint32_t c0 = slot_position(0);
    c1 = slot_position(MLA_STEP);
    c2 = slot_position(2 * MLA_STEP);
    const int32_t page0 = position_page(c0);
    page1 = position_page(c1);
    nextBits = issue_loads(c0, page0);
  }
  while (key0 < end) {   // (the same trips for every wave: the barrier below is met by all)
    const ListedKeys keys{nextBits};   // one mask for every tile: the heads of a row share its list
    // ---- the wave's partial S^T = K Q^T over its 144 columns, one per tile: s[t][r] = slot key0 + crow(r, hi), head of lane q of tile t
    f32x16 s[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
      for (int k = 0; k < MLA_NKS; ++k) s[t] = F::mfma(__builtin_bit_cast(v8, kreg[k]), qf[t][k], s[t]);
    }
    // ---- the latent fragments to the wave's image, once for every tile
#pragma unroll
    for (int k = 0; k < 8; ++k) *reinterpret_cast<u32x4 *>(Vs + ((k >> 1) * MLA_STEP + q) * 64 + (k & 1) * 32 + hi * 16) = kreg[k];
    // ---- the registers are free: the next step's rows fly during the rest of this one, behind them the page of the step after it
    // and the positions of the step after that
    key0 += MLA_STEP;
    if (key0 < end) {
      nextBits = issue_loads(c1, page1);
      c1 = c2;
      page1 = position_page(c1);
      c2 = slot_position(key0 + 2 * MLA_STEP);
    }

    // ---- the partials meet: [buffer][tile][wave][4][64 lanes] float4
    float4 *xb = reinterpret_cast<float4 *>(xchg + buf * XBUF);
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        xb[((t * MLA_WAVES + wave) * 4 + g) * 64 + lane] = make_float4(s[t][4 * g], s[t][4 * g + 1], s[t][4 * g + 2], s[t][4 * g + 3]);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if constexpr (TILES > 1) __builtin_amdgcn_sched_barrier(0);   // (four reads in flight at a time, as attn_mla16_prefill.h)
        const float4 *xt = xb + (t * MLA_WAVES * 4 + g) * 64 + lane;
        const float4 x0 = xt[0 * 4 * 64], x1 = xt[1 * 4 * 64], x2 = xt[2 * 4 * 64], x3 = xt[3 * 4 * 64];
        s[t][4 * g] = ((x0.x + x1.x) + x2.x) + x3.x;
        s[t][4 * g + 1] = ((x0.y + x1.y) + x2.y) + x3.y;
        s[t][4 * g + 2] = ((x0.z + x1.z) + x2.z) + x3.z;
        s[t][4 * g + 3] = ((x0.w + x1.w) + x2.w) + x3.w;
      }
    }
    buf ^= 1u;

    // ---- online softmax over the step's valid slots only, per tile: the same arithmetic on the same values in every wave
    v8 pf[TILES][2];
    float mx[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) mx[t] = score_max<true>(s[t], keys, 0u, hi, a.scale2);
#pragma unroll
    for (int t = 0; t < TILES; ++t) rescale_row_uniform(mx[t], m[t], l[t], o[t]);
#pragma unroll
    for (int t = 0; t < TILES; ++t) l[t] += score_exp<T, true>(s[t], keys, 0u, hi, m[t], pf[t]);

    // ---- O^T += V^T P^T over the wave's 128 latent columns, every tile from the one image
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int db = 0; db < MLA_NDB; ++db) o[t][db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[t][u], o[t][db]);
  }

  // ---- the end is the sparse decode body's, per tile, with the lane's head and the workgroup's row (no barrier follows)
#pragma unroll
  for (int t = 0; t < TILES; ++t) {
    const float l_tot = l[t] + __shfl_xor(l[t], 32);
    if (hp[t] >= H) continue;
    const float mult = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // a row without a visible slot: O = 0
    const int64_t at0 = (int64_t)batch * a.bso + (int64_t)head[t] * a.hso + (int64_t)qrow * a.ldo;
#pragma unroll
    for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = MLA_LATENT * wave + 32 * db + 8 * g + 4 * hi;
        const float4 x = make_float4(o[t][db][4 * g] * mult, o[t][db][4 * g + 1] * mult, o[t][db][4 * g + 2] * mult, o[t][db][4 * g + 3] * mult);
        store_o4<T>(a.o, at0 + d, a.outF32, x);
      }
    if (wave == 0 && hi == 0 && a.l) a.l[(int64_t)batch * a.lbs + (int64_t)head[t] * a.lhs + qrow] = row_lse(m[t], l_tot);
  }
}

} // namespace mfa
