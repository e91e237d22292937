// attn_fwd16_p4p.hip -- instantiations and launcher of the persistent four-wave forward kernel (attn_fwd16_p4p.h).
#include "attn_fwd16_p4p.h"
#include "launchers.h"

#include <cstdlib>
#include <cstring>

namespace mfa {

// sleep steps (x 512 clocks) per unit of (workgroup >> 3) & 31 in front of a workgroup's first block
#ifndef P4P_STAGGER
#define P4P_STAGGER 0
#endif

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
  constexpr bool CAUSAL = p4p::traits(STREAM).causal;
  constexpr uint64_t PER_UNIT = CAUSAL ? 2 : 1;
  const uint64_t total = (uint64_t)(CAUSAL ? (grid.x + 1) / 2 : grid.x) * grid.y * grid.z * splits;
  // one workgroup per compute unit; more only when a workgroup's share would not fit the block table.  A multiple of 8 keeps
  // fwd16_decode_block's head -> XCD affinity for every block of a workgroup
  uint64_t groups = total < (uint64_t)cus ? total : (uint64_t)cus;
  constexpr uint64_t MAX_UNITS = (p4p::TABLE_ENTRIES - 1) / PER_UNIT;   // (the table's last word holds the block count)
  if ((total + groups - 1) / groups > MAX_UNITS) groups = (total + MAX_UNITS - 1) / MAX_UNITS;
  if (groups >= 8) groups = (groups + 7) / 8 * 8;
  if (groups > total) groups = total;   // (so every workgroup's share fits the table)
  Fwd16Grid g{grid.x, grid.y, grid.z, splits, l.wsO, l.wsML};
  uint32_t stagger = P4P_STAGGER;
#ifdef MFA_DEV_VARIANTS
  if (const char *e = std::getenv("MFA_P4P_STAGGER")) stagger = (uint32_t)std::atoi(e);
#endif
  l.start(&attn_fwd16_p4p<T, STREAM>, dim3((uint32_t)groups), dim3(256), p4p::LDS_BYTES, l.args, g, (uint32_t)total, stagger);
  return form;
}

}  // namespace

// Dense launch of a D <= 128 forward problem on the persistent kernel: the launch form's text, nullptr when the launch is not one it
// serves (the caller then launches attn_fwd16_p4): block masks, a storage type of O / L no stream was generated for.
template <typename T, bool FOLD> const char *launch_p4p(const Launch &l) {
  const KernelArgs &args = l.args;
  if (args.mask) return nullptr;
  if (args.causal && args.C < args.R) return nullptr;
  // per-batch lengths (round 6): the causal ("geometry") streams carry the rows and keys of a block's batch entry in its table entry and
  // serve such launches with or without the causal mask (KernelArgs.causal is the stream's flag).  Without the mask they win (+4 % on
  // full-length batches, +1 % on mixed lengths against the one-block-per-workgroup kernel; interleaved rounds, profiles/r06_final/
  // time_varlen_d128.txt); WITH it a workgroup's fixed share of (long, short) row-block pairs is 6 % slower on mixed lengths than what
  // the dispatcher balances block by block (+4 % on full-length batches, which the host cannot tell apart: the lengths are device
  // arrays) -- causal launches with lengths stay with attn_fwd16_p4; the developer library routes them here with MFA_P4P_LENGTHS=1
  bool lengths_here = !args.causal;
#ifdef MFA_DEV_VARIANTS
  lengths_here = lengths_here || std::getenv("MFA_P4P_LENGTHS") != nullptr;
#endif
  if ((args.rowLen || args.colLen) && !lengths_here) return nullptr;
  const bool geometry = args.causal || args.rowLen || args.colLen;
  const char *form = (args.rowLen || args.colLen)
      ? (args.causal ? "attn_fwd16_p4p (persistent: one workgroup per compute unit walks the row-block pairs; per-batch lengths in the block table)"
                     : "attn_fwd16_p4p (persistent: one workgroup per compute unit walks the row-block pairs; per-batch lengths in the block table, no causal mask)")
      : (args.causal ? "attn_fwd16_p4p (persistent: one workgroup per compute unit walks the row-block pairs)"
                     : "attn_fwd16_p4p (persistent: one workgroup per compute unit walks the row blocks)");
#ifdef MFA_DEV_VARIANTS   // developer builds: A/B against the one-block-per-workgroup kernel, phase clocks (tools/p4p_prof.py)
  if (std::getenv("MFA_P4_NO_PERSISTENT")) return nullptr;
  if constexpr (!FOLD && __is_same(T, __bf16)) {
    if (std::getenv("MFA_P4P_PROF") && args.op[SLOT_O].precision == PREC_FP32 && args.op[SLOT_L].precision == PREC_FP32)
      return launch_stream<T, p4p::S_BF16_EXACT_PROF>(l, form);
  }
  // MFA_P4P_DEV_STREAM=<name of a developer stream of tools/p4pgen.py>: dense bf16 launches with FP32 O whose mode (mixed: FP16 L;
  // fp32 intermediates: FP32 L) the stream was generated for run that stream (schedule experiments and timing-only ablations,
  // tools/p4p_streams_ab.py)
  if constexpr (__is_same(T, __bf16)) {
    const char *want = std::getenv("MFA_P4P_DEV_STREAM");
    if (want && *want && args.op[SLOT_O].precision == PREC_FP32 && args.op[SLOT_L].precision == (FOLD ? PREC_FP16 : PREC_FP32)) {
#define MFA_P4P_BYNAME(name, f16, fold, o16, l16, scausal) \
      if constexpr (!f16 && fold == FOLD && !o16 && l16 == FOLD) { if (((scausal) & 3) != 2 && (((scausal) & 3) != 0) == geometry && std::strcmp(want, #name) == 0) return launch_stream<T, p4p::S_##name>(l, form); }
      MFA_P4P_DEV_STREAM_LIST(MFA_P4P_BYNAME)
#undef MFA_P4P_BYNAME
      return nullptr;   // (an unknown name must not silently time the product stream)
    }
  }
#endif
  const int po = args.op[SLOT_O].precision, pl = args.op[SLOT_L].precision;
  constexpr int PT = __is_same(T, _Float16) ? PREC_FP16 : PREC_BF16;
  const bool o16 = po == PT, l16 = pl == PREC_FP16;
  if (!o16 && po != PREC_FP32) return nullptr;
  if (!l16 && pl != PREC_FP32) return nullptr;
  if constexpr (FOLD) {
    if (!l16) return nullptr;   // (FOLD streams exist with FP16 L: the mixed-precision mode's storage type)
    if constexpr (__is_same(T, _Float16)) {
      if (geometry) return o16 ? launch_stream<T, p4p::S_F16_FOLD_O16_L16_CAUSAL>(l, form) : launch_stream<T, p4p::S_F16_FOLD_L16_CAUSAL>(l, form);
      return o16 ? launch_stream<T, p4p::S_F16_FOLD_O16_L16>(l, form) : launch_stream<T, p4p::S_F16_FOLD_L16>(l, form);
    } else {
      if (geometry) return o16 ? launch_stream<T, p4p::S_BF16_FOLD_O16_L16_CAUSAL>(l, form) : launch_stream<T, p4p::S_BF16_FOLD_L16_CAUSAL>(l, form);
      return o16 ? launch_stream<T, p4p::S_BF16_FOLD_O16_L16>(l, form) : launch_stream<T, p4p::S_BF16_FOLD_L16>(l, form);
    }
  } else {
    if (l16) return nullptr;
    if constexpr (__is_same(T, _Float16)) {
      if (geometry) return o16 ? launch_stream<T, p4p::S_F16_EXACT_O16_CAUSAL>(l, form) : launch_stream<T, p4p::S_F16_EXACT_CAUSAL>(l, form);
      return o16 ? launch_stream<T, p4p::S_F16_EXACT_O16>(l, form) : launch_stream<T, p4p::S_F16_EXACT>(l, form);
    } else {
      if (geometry) return o16 ? launch_stream<T, p4p::S_BF16_EXACT_O16_CAUSAL>(l, form) : launch_stream<T, p4p::S_BF16_EXACT_CAUSAL>(l, form);
      return o16 ? launch_stream<T, p4p::S_BF16_EXACT_O16>(l, form) : launch_stream<T, p4p::S_BF16_EXACT>(l, form);
    }
  }
}

// Column-parallel launch (few-workgroup problems: one head -- the reference's own benchmark shape): the pieces of the key range on the
// persistent kernel's split streams (round 6); the caller launches attn_fwd_combine behind it.  nullptr = not one it serves (pieces
// that are not whole multiples of two tiles): the caller launches the one-block-per-workgroup kernel's pieces
template <typename T, bool FOLD> const char *launch_p4p_split(const Launch &l) {
  const KernelArgs &args = l.args;
  if (args.rowLen || args.colLen || args.mask || args.causal || l.splits < 2) return nullptr;
  if (args.C % (128u * l.splits) != 0) return nullptr;
#ifdef MFA_DEV_VARIANTS
  if (std::getenv("MFA_P4_NO_PERSISTENT") || std::getenv("MFA_P4P_NO_SPLIT")) return nullptr;
#endif
  const char *form = "pieces by attn_fwd16_p4p, persistent";
  if constexpr (__is_same(T, _Float16))
    return FOLD ? launch_stream<T, p4p::S_F16_FOLD_SPLIT>(l, form) : launch_stream<T, p4p::S_F16_EXACT_SPLIT>(l, form);
  else
    return FOLD ? launch_stream<T, p4p::S_BF16_FOLD_SPLIT>(l, form) : launch_stream<T, p4p::S_BF16_EXACT_SPLIT>(l, form);
}
template const char *launch_p4p_split<__bf16, true>(const Launch &);
template const char *launch_p4p_split<__bf16, false>(const Launch &);
template const char *launch_p4p_split<_Float16, true>(const Launch &);
template const char *launch_p4p_split<_Float16, false>(const Launch &);
template const char *launch_p4p<__bf16, true>(const Launch &);
template const char *launch_p4p<__bf16, false>(const Launch &);
template const char *launch_p4p<_Float16, true>(const Launch &);
template const char *launch_p4p<_Float16, false>(const Launch &);

} // namespace mfa
