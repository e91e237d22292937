// attn_fwd16_p6.hip -- instantiations and launcher of the persistent D <= 64 forward kernel (attn_fwd16_p6.h).
#include "attn_fwd16_p6.h"
#include "launchers.h"

#include <cstdlib>
#include <cstring>

namespace mfa {

namespace {

// starts one stream (when l.run) and returns `form`: once a stream is chosen, a failed HIP call is the launch's error (l.err), nothing
// else runs instead
template <typename T, int STREAM> const char *launch_stream(const Launch &l, const char *form) {
  if (!l.run || l.err != hipSuccess) return form;
  int cus = 0;
  l.err = compute_units(&cus);
  if (l.err != hipSuccess) return form;
  const dim3 grid = l.grid;
  const uint32_t splits = l.splits;
  // units: row blocks, or (causal) pairs of row blocks -- two table entries each
  constexpr bool CAUSAL = p6::traits(STREAM).causal;
  constexpr uint64_t PER_UNIT = CAUSAL ? 2 : 1;
  const uint64_t total = (uint64_t)(CAUSAL ? (grid.x + 1) / 2 : grid.x) * grid.y * grid.z * splits;
  // one workgroup per compute unit; more only when a workgroup's share would not fit the block table.  A multiple of 8 keeps
  // fwd16_decode_block's head -> XCD affinity for every block of a workgroup
  uint64_t groups = total < (uint64_t)cus ? total : (uint64_t)cus;
  constexpr uint64_t MAX_UNITS = (p6::TABLE_ENTRIES - 1) / PER_UNIT;   // (the table's last word holds the block count)
  if ((total + groups - 1) / groups > MAX_UNITS) groups = (total + MAX_UNITS - 1) / MAX_UNITS;
  if (groups >= 8) groups = (groups + 7) / 8 * 8;
  if (groups > total) groups = total;   // (so every workgroup's share fits the table)
  Fwd16Grid g{grid.x, grid.y, grid.z, splits, l.wsO, l.wsML};
  l.start(&attn_fwd16_p6<T, STREAM>, dim3((uint32_t)groups), dim3(256), p6::LDS_BYTES, l.args, g, (uint32_t)total);
  return form;
}

bool serves(int precision, bool fold, const KernelArgs &args) {
  if (precision != PREC_BF16 && precision != PREC_FP16) return false;
  if (args.mask) return false;   // (per-batch lengths: served since round 6 -- the causal streams read rows / keys per block-table entry)
  if (args.causal && args.C < args.R) return false;
  if (args.D > 64 || args.D % 8) return false;
  const int po = args.op[SLOT_O].precision, pl = args.op[SLOT_L].precision;
  if (po != precision && po != PREC_FP32) return false;
  if (pl != (fold ? PREC_FP16 : PREC_FP32)) return false;   // (FOLD streams store FP16 L, the mixed-precision mode's type; EXACT ones FP32)
  for (int slot : {SLOT_Q, SLOT_K, SLOT_V, SLOT_O})
    if (args.op[slot].transposed) return false;
  return true;
}

}  // namespace

// Dense launch of a D <= 64 forward problem on the persistent kernel: the launch form's text, nullptr = not one it serves (the caller
// launches attn_fwd16_v3)
static const char *launch_p6(int precision, bool fold, const Launch &l) {
  const KernelArgs &args = l.args;
  if (!serves(precision, fold, args)) return nullptr;
  const char *form =
      (args.rowLen || args.colLen)
          ? (fold ? "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row-block pairs; per-batch lengths in the block table; row sums in the matrix pipe)"
                  : "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row-block pairs; per-batch lengths in the block table)")
      : args.causal ? (fold ? "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row-block pairs; row sums in the matrix pipe)"
                            : "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row-block pairs)")
                    : (fold ? "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row blocks; row sums in the matrix pipe)"
                            : "attn_fwd16_p6 (persistent: one workgroup per compute unit walks the row blocks)");
#ifdef MFA_DEV_VARIANTS
  if (std::getenv("MFA_P6_OFF")) return nullptr;
  if (const char *want = std::getenv("MFA_P6_DEV_STREAM")) {
    if (*want && precision == PREC_BF16 && args.op[SLOT_O].precision == PREC_FP32) {
#define MFA_P6_BYNAME(name, f16, sfold, o16, l16, scausal, ssplit) \
      if constexpr (!f16 && !o16 && !ssplit) { if ((sfold != 0) == fold && (scausal != 0) == (args.causal != 0 || args.rowLen || args.colLen) && std::strcmp(want, #name) == 0) return launch_stream<__bf16, p6::S_##name>(l, form); }
      MFA_P6_DEV_STREAM_LIST(MFA_P6_BYNAME)
#undef MFA_P6_BYNAME
      return nullptr;
    }
  }
#endif
  const bool o16 = args.op[SLOT_O].precision != PREC_FP32;
#define MFA_P6_PICK(T, PFX)                                                                                                          \
  if (args.causal || args.rowLen || args.colLen) {   /* the "geometry" streams; KernelArgs.causal is their run-time flag */           \
    if (fold) return o16 ? launch_stream<T, p6::S_##PFX##_FOLD_O16_L16_CAUSAL>(l, form) : launch_stream<T, p6::S_##PFX##_FOLD_L16_CAUSAL>(l, form); \
    return o16 ? launch_stream<T, p6::S_##PFX##_EXACT_O16_CAUSAL>(l, form) : launch_stream<T, p6::S_##PFX##_EXACT_CAUSAL>(l, form); \
  }                                                                                                                                  \
  if (fold) return o16 ? launch_stream<T, p6::S_##PFX##_FOLD_O16_L16>(l, form) : launch_stream<T, p6::S_##PFX##_FOLD_L16>(l, form); \
  return o16 ? launch_stream<T, p6::S_##PFX##_EXACT_O16>(l, form) : launch_stream<T, p6::S_##PFX##_EXACT>(l, form);
  if (precision == PREC_BF16) { MFA_P6_PICK(__bf16, BF16) }
  MFA_P6_PICK(_Float16, F16)
#undef MFA_P6_PICK
}

// Column-parallel launch (few-workgroup problems: one head, BASELINE config 2 as written): pieces of the key range on the persistent
// kernel, then the combine pass.  nullptr = not one it serves (pieces that are not whole multiples of four tiles, ...): the caller
// launches the eight-wave kernel's split sibling
static const char *launch_p6_split(int precision, bool fold, const Launch &l) {
  const KernelArgs &args = l.args;
  if (!serves(precision, fold, args) || args.causal || args.rowLen || args.colLen || l.splits < 2) return nullptr;
  if (args.C % (256u * l.splits) != 0) return nullptr;
#ifdef MFA_DEV_VARIANTS
  if (std::getenv("MFA_P6_OFF") || std::getenv("MFA_P6_NO_SPLIT")) return nullptr;
#endif
  const char *form = "pieces by attn_fwd16_p6, persistent";
  if (precision == PREC_BF16 && fold) launch_stream<__bf16, p6::S_BF16_FOLD_SPLIT>(l, form);
  else if (precision == PREC_BF16) launch_stream<__bf16, p6::S_BF16_EXACT_SPLIT>(l, form);
  else if (fold) launch_stream<_Float16, p6::S_F16_FOLD_SPLIT>(l, form);
  else launch_stream<_Float16, p6::S_F16_EXACT_SPLIT>(l, form);
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, l.wsML};
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * args.R;
  l.start(&attn_fwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, args, g);
  return form;
}

// the eight-wave kernel's launchers (attn_fwd16_v3.hip) for the launches this kernel does not serve
const char *fwd16_v3_d64_launch(int precision, const Launch &l);
const char *fwd16_v3_d64_launch_causal(int precision, const Launch &l);
const char *fwd16_v3_d64_launch_split(int precision, const Launch &l);

template <int PREC, bool FOLD, bool CAUSAL> static const char *launch_p6_or_v3(const Launch &l) {
  if (const char *form = launch_p6(PREC, FOLD, l)) return form;
  if (CAUSAL) fwd16_v3_d64_launch_causal(PREC, l);
  else fwd16_v3_d64_launch(PREC, l);
  // (the name rocprofv3 shows is the eight-wave kernel's)
  if (PREC == PREC_BF16)
    return CAUSAL ? "attn_fwd16v3_bf16_d64_w8x32_thr8 causal (eight-wave kernel: the launch is not one attn_fwd16_p6 serves)"
                  : "attn_fwd16v3_bf16_d64_w8x32_thr8 (eight-wave kernel: the launch is not one attn_fwd16_p6 serves)";
  return CAUSAL ? "attn_fwd16v3_f16_d64_w8x32_thr8 causal (eight-wave kernel: the launch is not one attn_fwd16_p6 serves)"
                : "attn_fwd16v3_f16_d64_w8x32_thr8 (eight-wave kernel: the launch is not one attn_fwd16_p6 serves)";
}
template <int PREC, bool FOLD> static const char *launch_p6_or_v3_split(const Launch &l) {
  if (const char *pieces = launch_p6_split(PREC, FOLD, l)) return pieces;
  fwd16_v3_d64_launch_split(PREC, l);
  return PREC == PREC_BF16 ? "pieces by the eight-wave kernel attn_fwd16v3_bf16_d64_w8x32_thr8 (not a split attn_fwd16_p6 serves)"
                           : "pieces by the eight-wave kernel attn_fwd16v3_f16_d64_w8x32_thr8 (not a split attn_fwd16_p6 serves)";
}

template <int PREC, bool FOLD> static void attach(VariantInfo *v) {
  v->dense = v->own(&launch_p6_or_v3<PREC, FOLD, false>);
  v->causal = v->own(&launch_p6_or_v3<PREC, FOLD, true>);
  v->split = v->own(&launch_p6_or_v3_split<PREC, FOLD>, 256);   // one workgroup per compute unit
}

// `out` arrives filled by fwd16_v3_variant(precision, 64, 0): its block-sparse launches stay with that kernel, and so do the dense,
// causal and column-parallel launches this kernel does not serve (transposed operands, other storage types of L) -- in the same
// 256-row blocks, so that a launch handed over keeps its grid
bool fwd16_p6_variant(int precision, bool fold, VariantInfo *out) {
  if (precision != PREC_BF16 && precision != PREC_FP16) return false;
  if (out->dense.parallelization != 256 || out->split.parallelization != 256) return false;
  out->name = precision == PREC_BF16 ? (fold ? "attn_fwd16p6_bf16_d64_w4x64_thr8_fold" : "attn_fwd16p6_bf16_d64_w4x64_thr8")
                                     : (fold ? "attn_fwd16p6_f16_d64_w4x64_thr8_fold" : "attn_fwd16p6_f16_d64_w4x64_thr8");
  out->parallelization = 256;
  out->traversal = 64;
  out->headBlock = 64;
  out->threads = 256;
  out->ldsBytes = out->ldsBytes > (uint32_t)p6::LDS_BYTES ? out->ldsBytes : (uint32_t)p6::LDS_BYTES;
  if (precision == PREC_BF16) fold ? attach<PREC_BF16, true>(out) : attach<PREC_BF16, false>(out);
  else fold ? attach<PREC_FP16, true>(out) : attach<PREC_FP16, false>(out);
  return true;
}

} // namespace mfa
