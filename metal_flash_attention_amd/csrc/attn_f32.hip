// attn_f32.hip -- instantiations and launchers of the FP32 production kernels (attn_f32.h).  The variant's launcher takes a launch
// when f32k::serves() says its operands qualify and hands the others to the dense route of the general kernel
// (attn_generic_{fwd,dq,dkv}.hip); its return value names the code object that ran (mfa_attention_kernel_launch_form).
#include "attn_f32.h"
#include "launchers.h"

#include <cstdlib>

namespace mfa {

namespace {

template <int DP> void start(int type, const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  const dim3 flat(l.grid.x * l.grid.y * l.grid.z);
  switch (type) {
    case 0:
      l.start(&f32k::attn_f32_fwd<DP>, flat, dim3(256), f32k::lds_bytes<DP>(), l.args, g);
      return;
    case 1:
#ifdef MFA_DEV_VARIANTS   // MFA_F32_PROF=1: phase clocks instead of dQ (attn_f32.h, PROF)
      if constexpr (DP == 128) {
        if (std::getenv("MFA_F32_PROF")) { l.start(&f32k::attn_f32_dq<DP, true>, flat, dim3(256), f32k::lds_bytes_dq<DP>(), l.args, g); return; }
      }
#endif
      l.start(&f32k::attn_f32_dq<DP>, flat, dim3(256), f32k::lds_bytes_dq<DP>(), l.args, g);
      return;
    default:
      l.start(&f32k::attn_f32_dkv<DP>, flat, dim3(256), f32k::lds_bytes_dkv<DP>(), l.args, g);
      return;
  }
}

// the FP32 kernel when the operands qualify, else the general kernel of the head block: both in blocks of f32k::ROWS, heads, batches
template <int TYPE, int DP> const char *launch_f32(const Launch &l) {
  bool taken = f32k::serves(TYPE, DP, l.args);
#ifdef MFA_DEV_VARIANTS   // developer builds: MFA_F32_GENERAL=1 keeps the general kernels on these launches (A/B runs)
  if (std::getenv("MFA_F32_GENERAL")) taken = false;
#endif
  if (taken) {
    start<DP>(TYPE, l);
    return nullptr;   // (the variant's own name: the FP32 production kernel)
  }
  VariantInfo generic;
  (TYPE == 0 ? generic_fwd_variant : TYPE == 1 ? generic_dq_variant : generic_dkv_variant)(DP, &generic);
  generic.dense.launch(l);
  static const char *const general[3][2] = {
      {"attn_generic_fwd_f32mfma_d64_w4_cached (general kernel: an operand's rows are not 16-byte aligned)",
       "attn_generic_fwd_f32mfma_d128_w4_cached (general kernel: an operand's rows are not 16-byte aligned)"},
      {"attn_generic_dq_f32mfma_d64_w4_cached (general kernel: an operand's rows are not 16-byte aligned)",
       "attn_generic_dq_f32mfma_d128_w4_cached (general kernel: an operand's rows are not 16-byte aligned)"},
      {"attn_generic_dkv_f32mfma_d64_w4_cached (general kernel: an operand's rows are not 16-byte aligned)",
       "attn_generic_dkv_f32mfma_d128_w4_cached (general kernel: an operand's rows are not 16-byte aligned)"}};
  return general[TYPE][DP == 128];
}

template <int TYPE, int DP> void fill_f32(VariantInfo *v) {
  static const char *const names[3][2] = {{"attn_f32_fwd_d64_w4x32", "attn_f32_fwd_d128_w4x32"},
                                          {"attn_f32_dq_d64_w4x32", "attn_f32_dq_d128_w4x32"},
                                          {"attn_f32_dkv_d64_w4x32", "attn_f32_dkv_d128_w4x32"}};
  v->name = names[TYPE][DP == 128];
  v->ldsBytes = TYPE == 0 ? f32k::lds_bytes<DP>() : TYPE == 1 ? f32k::lds_bytes_dq<DP>() : f32k::lds_bytes_dkv<DP>();
  v->dense = v->causal = v->own(&launch_f32<TYPE, DP>);   // (block-sparse launches keep the general kernel's route)
}

}  // namespace

bool f32_variant(int type, int DP, VariantInfo *out) {
  if ((DP != 64 && DP != 128) || out->dense.parallelization != f32k::ROWS) return false;
  switch (type) {
    case 0: if (DP == 64) fill_f32<0, 64>(out); else fill_f32<0, 128>(out); break;
    case 1: if (DP == 64) fill_f32<1, 64>(out); else fill_f32<1, 128>(out); break;
    default: if (DP == 64) fill_f32<2, 64>(out); else fill_f32<2, 128>(out); break;
  }
  return true;
}

}  // namespace mfa
