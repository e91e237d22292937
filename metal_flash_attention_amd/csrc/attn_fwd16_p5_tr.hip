// attn_fwd16_p5_tr.hip -- instantiations of the hand-placed forward kernel for transposed K and / or V at the head-dimension
// buckets 160 / 192 / 256 (attn_fwd16_p5_tr.h) and the launcher that prefers it over the 8 x 32 kernel's transposed code object
// when the launch is whole 32-key steps of aligned rows -- the same arrangement as attn_fwd16_p4_tr.hip at D <= 128.
// GPU evidence (round 4, all patterns): tests/test_attention_gpu.py::test_forward_stream_reads_transposed_keys_and_values_at_large_head_dimensions,
// profiles/r04_candidate/time_p5_tr_32heads.txt.
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "attn_fwd16_p5_tr.h"
#include "launchers.h"

namespace mfa {

// what the step walk of attn_fwd16_p5_tr needs (its header): K / V transposed as the stream's pattern says (bit 0 = K, bit 1 = V),
// no per-batch lengths, no block mask, whole 32-key steps, 16-byte aligned rows of K and V in either orientation (and of Q when
// it is row-major: its fragments are 8- or 16-byte loads; Q^T is gathered)
static bool p5_tr_takes(const KernelArgs &a, int pattern) {
#ifdef MFA_DEV_VARIANTS
  const char *knob = std::getenv("MFA_FWD16_P5_TR");   // developer library: MFA_FWD16_P5_TR=0 keeps the 8 x 32 code object (A/B runs)
  if (knob && std::strcmp(knob, "0") == 0) return false;
#endif
  auto aligned = [](const OperandView &v) {
    return ((reinterpret_cast<uintptr_t>(v.ptr) | (uint64_t)v.ld * 2 | (uint64_t)v.headStride * 2 | (uint64_t)v.batchStride * 2) & 15) == 0;
  };
  if (a.rowLen || a.colLen || a.mask || a.D <= 128 || a.D > 256 || a.D % 8 || a.C % 32 || a.C == 0) return false;
  if (a.causal && a.C < a.R) return false;
  if ((a.op[SLOT_K].transposed != 0) != ((pattern & 1) != 0) || (a.op[SLOT_V].transposed != 0) != ((pattern & 2) != 0)) return false;
  if (!aligned(a.op[SLOT_K]) || !aligned(a.op[SLOT_V])) return false;   // (16-byte chunks of either orientation)
  return a.op[SLOT_Q].transposed || aligned(a.op[SLOT_Q]);
}

// the launch form's text of a launch the stream takes
template <int STREAM> static const char *stream_text() {
  constexpr int PATTERN = p5tr::stream_pattern(STREAM);
  if (PATTERN == 1)
    return p5tr::stream_folds(STREAM) ? "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed K; scale folded into Q)"
                                       : "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed K)";
  if (PATTERN == 2)
    return p5tr::stream_folds(STREAM) ? "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed V; scale folded into Q)"
                                       : "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed V)";
  return p5tr::stream_folds(STREAM) ? "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed K / V; scale folded into Q)"
                                     : "attn_fwd16_p5_tr (four waves x 64 rows, 32-key steps, hand-placed stream on transposed K / V)";
}

template <typename T, int STREAM>
static const char *launch_p5_tr(const Launch &l) {
  constexpr int D = p5tr::stream_bucket(STREAM), PATTERN = p5tr::stream_pattern(STREAM);
  if (!p5_tr_takes(l.args, PATTERN)) {   // the dense route of the transposed code object `out` arrived with (attn_fwd16_v3_tr_dNNN.hip)
    VariantInfo tr;
    fwd16_v3_tr_variant(std::is_same<T, __bf16>::value ? PREC_BF16 : PREC_FP16, D, PATTERN, &tr);
    return tr.dense.launch(l);
  }
  // l.grid counts the transposed code object's 128-row blocks; this kernel's take 256 rows
  const uint32_t blocks = ((uint32_t)l.args.R + 255) / 256;
  Fwd16Grid g{blocks, l.grid.y, l.grid.z};
  if (l.args.causal) {
    const uint32_t groups = (blocks + 1) / 2;   // one workgroup per pair of row blocks (last - i, i)
    l.start(&attn_fwd16_p5_tr<T, STREAM, true>, dim3(groups * l.grid.y * l.grid.z), dim3(256), p5::LDS_BYTES, l.args, g);
  } else {
    l.start(&attn_fwd16_p5_tr<T, STREAM, false>, dim3(blocks * l.grid.y * l.grid.z), dim3(256), p5::LDS_BYTES, l.args, g);
  }
  return stream_text<STREAM>();
}

template <typename T, int STREAM> static void attach(VariantInfo *v) {
  v->dense = v->causal = v->own(&launch_p5_tr<T, STREAM>);   // (the causal mask: a run-time flag of both kernels)
  v->ldsBytes = v->ldsBytes > (uint32_t)p5::LDS_BYTES ? v->ldsBytes : (uint32_t)p5::LDS_BYTES;
}

// `out` arrives filled by fwd16_v3_tr_variant of the bucket for `pattern` (bit 0 = K, bit 1 = V transposed; 0 = only Q / O:
// nothing to do): launches the stream can take go to it, the others stay.  fold: Q pre-multiplied by the softmax scale in the 16-bit
// type (mixed-precision descriptors)
bool fwd16_p5_tr_variant(int precision, int bucket, int pattern, bool fold, VariantInfo *out) {
  if (!out->transposedInPlace) return false;
#define MFA_P5TR_ATTACH1(T, TN, B, SFX) { if (fold) attach<T, p5tr::S_D##B##_##TN##_FOLD_##SFX>(out); else attach<T, p5tr::S_D##B##_##TN##_THR8_##SFX>(out); return true; }
#define MFA_P5TR_ATTACH(T, TN, SFX)                \
  switch (bucket) {                                \
    case 160: MFA_P5TR_ATTACH1(T, TN, 160, SFX)    \
    case 192: MFA_P5TR_ATTACH1(T, TN, 192, SFX)    \
    case 256: MFA_P5TR_ATTACH1(T, TN, 256, SFX)    \
    default: return false;                         \
  }
#ifdef MFA_P5_TR1_STREAMS   // (the one-operand streams are generated at build time, attn_fwd16_p5_tr.h)
#define MFA_P5TR_ONE_OPERAND(T, TN) case 1: MFA_P5TR_ATTACH(T, TN, TRK) case 2: MFA_P5TR_ATTACH(T, TN, TRV)
#else
#define MFA_P5TR_ONE_OPERAND(T, TN)
#endif
#define MFA_P5TR_PATTERNS(T, TN)                   \
  switch (pattern) {                               \
    MFA_P5TR_ONE_OPERAND(T, TN)                    \
    case 3: MFA_P5TR_ATTACH(T, TN, TR)             \
    default: return false;                         \
  }
  if (precision == PREC_BF16) { MFA_P5TR_PATTERNS(__bf16, BF16) }
  if (precision == PREC_FP16) { MFA_P5TR_PATTERNS(_Float16, F16) }
#undef MFA_P5TR_PATTERNS
#undef MFA_P5TR_ONE_OPERAND
#undef MFA_P5TR_ATTACH
#undef MFA_P5TR_ATTACH1
  return false;
}

} // namespace mfa
