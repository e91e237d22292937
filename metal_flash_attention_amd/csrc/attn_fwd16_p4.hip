// attn_fwd16_p4.hip -- instantiations of the four-wave, 64-rows-per-wave forward kernel (attn_fwd16_p4.h).
#include "attn_fwd16_p4.h"
#include "launchers.h"

namespace mfa {

// persistent form (attn_fwd16_p4p.hip): the launch form's text of the launches it serves (started when l.run), nullptr = not served
template <typename T, bool FOLD> const char *launch_p4p(const Launch &l);
template <typename T, bool FOLD> const char *launch_p4p_split(const Launch &l);

template <int STREAM> constexpr bool has_persistent() {
  return STREAM == p4::S_BF16_THR8 || STREAM == p4::S_F16_THR8 || STREAM == p4::S_BF16_FOLD || STREAM == p4::S_F16_FOLD;
}

template <typename T, int STREAM, bool CAUSAL>
static const char *launch_p4(const Launch &l) {
  if constexpr (has_persistent<STREAM>()) {
    if (const char *form = launch_p4p<T, p4::stream_folds(STREAM)>(l)) return form;   // (dense and causal)
  }
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  const uint32_t groups = CAUSAL ? (l.grid.x + 1) / 2 : l.grid.x;   // causal: one workgroup per pair of row blocks (last - i, i)
  l.start(&attn_fwd16_p4<T, STREAM, CAUSAL>, dim3(groups * l.grid.y * l.grid.z), dim3(256), p4::LDS_BYTES, l.args, g);
  return nullptr;
}

// column-parallel launch (few-workgroup problems: one head, long sequences): pieces of the key range, then the combine pass
template <typename T, int STREAM>
static const char *launch_p4_split(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, l.wsML};
  const char *pieces = nullptr;
  if constexpr (has_persistent<STREAM>())
    pieces = launch_p4p_split<T, p4::stream_folds(STREAM)>(l);   // (round 6: the pieces on the persistent kernel)
  if (!pieces) {
    pieces = "pieces by attn_fwd16_p4, one block per workgroup";
    l.start(&attn_fwd16_p4<T, STREAM, false, true>, dim3(l.grid.x * l.grid.y * l.grid.z * l.splits), dim3(256), p4::LDS_BYTES, l.args, g);
  }
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * l.args.R;
  l.start(&attn_fwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g);
  return pieces;
}

template <typename T, int STREAM> static void fill_p4(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = 256;
  v->traversal = 64;
  v->headBlock = 128;
  v->threads = 256;
  v->ldsBytes = v->ldsBytes > (uint32_t)p4::LDS_BYTES ? v->ldsBytes : (uint32_t)p4::LDS_BYTES;   // (siblings of the 8 x 32 kernel keep theirs)
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_p4<T, STREAM, false>);
  v->causal = v->own(&launch_p4<T, STREAM, true>);
  v->split = v->own(&launch_p4_split<T, STREAM>, 256);   // one workgroup per compute unit (block-sparse launches keep the 8 x 32 kernel's route)
}

template <typename T, int STREAM> static void fill_p4_dev(VariantInfo *v, const char *name) {   // dense launches only
  fill_p4<T, p4::S_BF16_THR8>(v, name);
  v->dense = v->own(&launch_p4<T, STREAM, false>);
  if constexpr (p4::stream_profiles(STREAM)) v->causal = v->own(&launch_p4<T, STREAM, true>);   // phase clocks of causal launches too (tools/p4_prof.py --causal)
  else v->causal = Route();
}

// Product streams: impl 0 = scale applied in fp32 (exact S; selected when the descriptor keeps the attention matrix in
// FP32 registers), impl 10 = FOLD (Q pre-multiplied by the softmax scale in the 16-bit type, the running maximum
// subtracted inside the matrix pipe; selected with lowPrecisionIntermediates, where the reference itself holds P -- and
// for FP16 also S -- in 16 bits), impl 1 = THR = 0 (the reference's rescale rule, +Softmax.swift:290-301, instead of the
// deferred one).  Everything else is a developer stream (libmfa_hip_dev.so only): MFA_FWD16_IMPL=p4:<1000 + stream index>
// for A/B placements, phase-clock stamps and timing-only ablations (tools/p4_prof.py lists the indices).
bool fwd16_p4_variant(int precision, int D, int impl, VariantInfo *out) {
  if (D != 128) return false;
  if (precision == PREC_BF16) {
    if (impl == 0) { fill_p4<__bf16, p4::S_BF16_THR8>(out, "attn_fwd16p4_bf16_d128_w4x64_thr8"); return true; }
#ifdef MFA_DEV_VARIANTS   // (no descriptor selects the THR = 0 stream: developer library only, MFA_FWD16_IMPL=p4:1)
    if (impl == 1) { fill_p4<__bf16, p4::S_BF16_THR0>(out, "attn_fwd16p4_bf16_d128_w4x64_thr0"); return true; }
#endif
    if (impl == 10) { fill_p4<__bf16, p4::S_BF16_FOLD>(out, "attn_fwd16p4_bf16_d128_w4x64_thr8_fold"); return true; }
#ifdef MFA_DEV_VARIANTS
#define MFA_P4_DEV(name) if (impl == 1000 + p4::S_##name) { fill_p4_dev<__bf16, p4::S_##name>(out, "attn_fwd16p4_DEV_" #name); return true; }
    MFA_P4_DEV_STREAM_LIST(MFA_P4_DEV)
#undef MFA_P4_DEV
#endif
  }
  if (precision == PREC_FP16) {
    if (impl == 0) { fill_p4<_Float16, p4::S_F16_THR8>(out, "attn_fwd16p4_f16_d128_w4x64_thr8"); return true; }
    if (impl == 10) { fill_p4<_Float16, p4::S_F16_FOLD>(out, "attn_fwd16p4_f16_d128_w4x64_thr8_fold"); return true; }
  }
  return false;
}

} // namespace mfa
