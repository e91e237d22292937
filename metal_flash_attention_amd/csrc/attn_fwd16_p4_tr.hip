// attn_fwd16_p4_tr.hip -- instantiations of the hand-placed forward kernel for transposed K and / or V (attn_fwd16_p4_tr.h) and the
// launcher that prefers it over the 8 x 32 kernel's transposed code object when the launch is whole chunks of aligned rows.
#include "attn_fwd16_p4_tr.h"
#include "attn_fwd16_v3_launch.h"

namespace mfa {

// what the tile walk of attn_fwd16_p4_tr needs (its header): no per-batch lengths, no block mask, 16-byte aligned rows of the
// transposed operands (K^T, V^T and, if transposed, Q^T), whole 16-byte chunks of keys in V^T (the last tile's chunks at or beyond
// key C are left out, a chunk cannot be cut); row-major operands as the row-major kernel wants them (checked before)
static bool p4_tr_takes(const KernelArgs &a, int pattern) {
  if (a.rowLen || a.colLen || a.mask) return false;
  auto aligned = [](const OperandView &v) {
    return ((reinterpret_cast<uintptr_t>(v.ptr) | (uint64_t)v.ld * 2 | (uint64_t)v.headStride * 2 | (uint64_t)v.batchStride * 2) & 15) == 0;
  };
  if ((a.op[SLOT_K].transposed != 0) != ((pattern & 1) != 0) || (a.op[SLOT_V].transposed != 0) != ((pattern & 2) != 0)) return false;
  if ((pattern & 2) && a.C % 8 != 0) return false;
  return aligned(a.op[SLOT_K]) && aligned(a.op[SLOT_V]) && aligned(a.op[SLOT_Q]);
}

// the launch form's text of a launch the stream takes
template <int STREAM> static const char *stream_text() {
  constexpr int PATTERN = p4tr::stream_pattern(STREAM);
  if (PATTERN == 3)
    return p4tr::stream_folds(STREAM) ? "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed K / V; scale folded into Q)"
                                       : "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed K / V)";
  if (PATTERN == 1)
    return p4tr::stream_folds(STREAM) ? "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed K; scale folded into Q)"
                                       : "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed K)";
  return p4tr::stream_folds(STREAM) ? "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed V; scale folded into Q)"
                                     : "attn_fwd16_p4_tr (four waves x 64 rows, hand-placed stream on transposed V)";
}

template <typename T, int STREAM>
static const char *launch_p4_tr(const Launch &l) {
  constexpr int PATTERN = p4tr::stream_pattern(STREAM);
  // (l.grid counts 256-row blocks, the 8 x 32 kernel's and this kernel's: fwd16_p4_tr_variant)
  if (!p4_tr_takes(l.args, PATTERN)) return launch_v3_tr<T, 128, 8, 3, 0, 4 | PATTERN>(l);
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  if (l.args.causal) {
    const uint32_t groups = (l.grid.x + 1) / 2;   // one workgroup per pair of row blocks (last - i, i)
    l.start(&attn_fwd16_p4_tr<T, STREAM, true>, dim3(groups * l.grid.y * l.grid.z), dim3(256), p4::LDS_BYTES, l.args, g);
  } else {
    l.start(&attn_fwd16_p4_tr<T, STREAM, false>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(256), p4::LDS_BYTES, l.args, g);
  }
  return stream_text<STREAM>();
}

template <typename T, int STREAM> static void attach(VariantInfo *v) {
  v->dense = v->causal = v->own(&launch_p4_tr<T, STREAM>);   // (the causal mask: a run-time flag of both kernels)
  v->ldsBytes = v->ldsBytes > (uint32_t)p4::LDS_BYTES ? v->ldsBytes : (uint32_t)p4::LDS_BYTES;
}

// `out` arrives filled by fwd16_v3_tr_variant at bucket 128 for `pattern` (bit 0 = K, bit 1 = V transposed; 0 = only Q / O: nothing to do):
// launches the stream can take go to it, the others stay.  fold: Q pre-multiplied by the softmax scale in the 16-bit type
// (mixed-precision descriptors).  The launches the stream does not take go to the 8 x 32 kernel in the same 256-row blocks
bool fwd16_p4_tr_variant(int precision, int pattern, bool fold, VariantInfo *out) {
  if (out->dense.parallelization != 256) return false;
#define MFA_P4TR_ATTACH(T, TN)                                                                        \
  switch (pattern) {                                                                                   \
    case 1: if (fold) attach<T, p4tr::S_##TN##_FOLD_TRK>(out); else attach<T, p4tr::S_##TN##_THR8_TRK>(out); return true; \
    case 2: if (fold) attach<T, p4tr::S_##TN##_FOLD_TRV>(out); else attach<T, p4tr::S_##TN##_THR8_TRV>(out); return true; \
    case 3: if (fold) attach<T, p4tr::S_##TN##_FOLD_TR>(out); else attach<T, p4tr::S_##TN##_THR8_TR>(out); return true;   \
    default: return false;                                                                             \
  }
  if (precision == PREC_BF16) { MFA_P4TR_ATTACH(__bf16, BF16) }
  if (precision == PREC_FP16) { MFA_P4TR_ATTACH(_Float16, F16) }
#undef MFA_P4TR_ATTACH
  return false;
}

} // namespace mfa
