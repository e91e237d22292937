// attn_mla16_sparse.h -- sparse MLA decode (include/mfa_mla_sparse.h): the decode of attn_mla16.h over a per-(sequence,
// row) LIST of key positions, shared by all heads, instead of over every key below the length.  A sibling body of mla_decode_body: a
// lane there already is one key row and issues its own nine 16-byte loads at its own address, so a list only changes where that address
// comes from.  The partition of the columns over the four waves, the exchange of the partial scores, both products, the 64 KiB LDS plan
// and the end are attn_mla16.h's, and so are its constants, rescale_row / score_max / score_exp / vt_mfma / store_o4 / row_lse and the
// combine body.  What is this body's own:
//
//   * packing.  The rows packed into a workgroup must share one list: a workgroup serves 32 HEADS (head = 32 group + q) of ONE
//     (sequence, row) and one piece of the list's SLOTS.  Grid: batches x rows x groups x pieces, pieces fastest, then the group.
//   * the key of a lane.  Lane q of step i reads slot begin + 32 i + q of the list (-1 at or past the piece's end), decides by itself
//     whether the position c is valid -- 0 <= c < min(len_b, column) and, causal, c <= row + max(len_b - R, 0): one unsigned comparison
//     against a wave-uniform limit -- and forms its own row address; paged: one block-table read per lane.  A hole is never loaded (its
//     row comes in as zeros), its table entry is never read and its score is replaced.
//   * visibility.  The low word of the wave's ballot of "valid" is the step's 32-bit mask (ListedKeys); score_max<true> and
//     score_exp<T, true> test its bit crow(r, hi) through cur = 0.  A step of 32 holes has mask 0: its maximum is -FLT_MAX, which never
//     exceeds m, every p is an exact 0 and the image holds zeros -- (m, l, O) stay bit for bit what they were.
//   * loads in flight.  The rows of step i + 1 are issued in the middle of step i, as in the dense body.  The one or two dependent
//     loads in front of them are fetched further ahead: step i issues the block-table read of step i + 2 and the index read of step
//     i + 3, so that an address is always formed from loads issued a whole step earlier.
#pragma once
#include "attn_mla16.h"

namespace mfa {

struct MlaSparseArgs {
  MlaArgs a;                 // groups = ceil(H / 32): the groups of heads of one (sequence, row); M = H R, the rows of a slab per sequence
  const int32_t *indices;    // [batches][rows][topk] key positions
  int64_t irs, ibs;          // entries between the lists of two rows / two sequences
  uint32_t topk;
};

// the keys of one step that a list names and the rule admits: bit j = the step's slot j
struct ListedKeys {
  uint32_t bits;
  __device__ __forceinline__ bool visible(uint32_t j) const { return (bits >> j) & 1u; }
};

template <typename T, bool SPLIT>
__device__ __forceinline__ void mla_sparse_decode_body(const MlaSparseArgs &sa) {
  typedef Frag16<T> F;
  typedef typename F::v8 v8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
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

  // ---- the lane's head; heads at or past H repeat the last one and are not stored
  const uint32_t hp = group * MLA_ROWS + (uint32_t)q;
  const uint32_t head = min(hp, H - 1);
  const int col0 = MLA_LATENT * wave + 8 * hi, colR = MLA_DV + MLA_ROPE * wave + 8 * hi;
  v8 qf[MLA_NKS];
  {
    const char *qp = a.q + ((int64_t)batch * a.bsq + (int64_t)head * a.hsq + (int64_t)qrow * a.ldq) * 2;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t)
      qf[t] = __builtin_bit_cast(v8, *reinterpret_cast<const u32x4 *>(qp + (t < 8 ? col0 + 16 * t : colR) * 2));
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

  // lane = the key row of slot q of the step, its slice of the row as the A operand; returns the step's mask
  u32x4 kreg[MLA_NKS];
  auto issue_loads = [&](uint32_t c, int32_t page) -> uint32_t {
    const bool kvalid = c < lim;
    const int64_t ko = a.paged ? (int64_t)page * a.psk + (int64_t)(c & pageMask) * a.ldk : (int64_t)batch * a.bsk + (int64_t)c * a.ldk;
    const char *kp = a.kv + ko * 2;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t) {
      u32x4 z = {0u, 0u, 0u, 0u};
      if (kvalid) z = *reinterpret_cast<const u32x4 *>(kp + (t < 8 ? col0 + 16 * t : colR) * 2);
      kreg[t] = z;
    }
    return (uint32_t)__ballot(kvalid);   // lanes 0 .. 31 are the step's slots
  };

  f32x16 o[MLA_NDB];
  float m = STEP_MINUS_HUGE, l = 0.f;
#pragma unroll
  for (int db = 0; db < MLA_NDB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  char *Vs = smem + wave * MLA_IMAGE;   // this wave's V image: [4 d blocks][32 keys][32 d]
  char *xchg = smem + MLA_WAVES * MLA_IMAGE;
  const int vtr_off = vtr_lane_offset(lane, hi);

  // ---- the pipeline's start: positions of the first three steps, pages of the first two, rows of the first
  uint32_t key0 = begin, buf = 0, nextBits = 0;
  uint32_t c1 = 0xFFFFFFFFu, c2 = 0xFFFFFFFFu;   // positions of the steps after this one and after that
  int32_t page1 = 0;                             // page of c1
  if (key0 < end) {
    const uint32_t c0 = slot_position(key0);
    c1 = slot_position(key0 + MLA_STEP);
    c2 = slot_position(key0 + 2 * MLA_STEP);
    const int32_t page0 = position_page(c0);
    page1 = position_page(c1);
    nextBits = issue_loads(c0, page0);
  }
  while (key0 < end) {   // (the same trips for every wave: the barrier below is met by all)
    const ListedKeys keys{nextBits};
    // ---- the wave's partial S^T = K Q^T over its 144 columns: s[r] = slot key0 + crow(r, hi), head of lane q
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < MLA_NKS; ++t) s = F::mfma(__builtin_bit_cast(v8, kreg[t]), qf[t], s);
    // ---- the latent fragments to the wave's image (attn_mla16.h)
#pragma unroll
    for (int t = 0; t < 8; ++t) *reinterpret_cast<u32x4 *>(Vs + ((t >> 1) * MLA_STEP + q) * 64 + (t & 1) * 32 + hi * 16) = kreg[t];
    // ---- the registers are free: the next step's rows fly during the rest of this one, behind them the page of the step after it
    // and the positions of the step after that
    key0 += MLA_STEP;
    if (key0 < end) {
      nextBits = issue_loads(c1, page1);
      c1 = c2;
      page1 = position_page(c1);
      c2 = slot_position(key0 + 2 * MLA_STEP);
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
    rescale_row(score_max<true>(s, keys, 0u, hi, a.scale2), m, l, o);
    v8 pf[2];
    l += score_exp<T, true>(s, keys, 0u, hi, m, pf);

    // ---- O^T += V^T P^T over the wave's 128 latent columns
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int db = 0; db < MLA_NDB; ++db) o[db] = vt_mfma<T>(Vs + (db * MLA_STEP + 16 * u) * 64 + vtr_off, pf[u], o[db]);
  }

  // ---- the end is the dense body's, with the lane's head and the workgroup's row
  const float l_tot = l + __shfl_xor(l, 32);
  if (hp >= H) return;   // (no barrier follows)
  float mult = 1.0f;
  if constexpr (!SPLIT) mult = l_tot > 0.f ? 1.0f / l_tot : 0.f;   // a row without a visible slot: O = 0
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
