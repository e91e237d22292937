// attn_dkv16_p4.hip -- instantiations of the four-wave, 64-keys-per-wave backwardKeyValue kernel (attn_dkv16_p4.h).
#include "attn_dkv16_p4.h"
#include "launchers.h"

namespace mfa {

template <typename T, int STREAM, bool CAUSAL>
static const char *launch_dkv_p4(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dkv16_p4<T, STREAM, CAUSAL>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(256), dkv4::LDS_BYTES, l.args, g);
  return nullptr;
}

// row-parallel launch: the 32-row steps in `splits` pieces (SPLIT of attn_dkv16_p4.h), then the sums of the dV and dK slabs
template <typename T, int STREAM>
static const char *launch_dkv_p4_split(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, nullptr};
  l.start(&attn_dkv16_p4<T, STREAM, false, true>, dim3(l.grid.x * l.grid.y * l.grid.z * l.splits), dim3(256), dkv4::LDS_BYTES, l.args, g);
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * l.args.C;
  const float *dk_slabs = l.wsO + (uint64_t)l.splits * rows * l.args.D;   // dV slabs first, then dK slabs
  l.start(&attn_bwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g, (int)SLOT_dV, l.args.C, (const float *)l.wsO);
  l.start(&attn_bwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g, (int)SLOT_dK, l.args.C, dk_slabs);
  return nullptr;
}

// `v` arrives filled by dkv16_rs_variant: block-sparse launches and causal row-parallel ones keep the role-split kernel's routes
template <typename T, int STREAM> static void fill_dkv_p4(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = 256;   // key columns per workgroup: four waves x 64
  v->traversal = 32;
  v->headBlock = dkv4::stream_bucket(STREAM);
  v->threads = 256;
  v->ldsBytes = v->ldsBytes > (uint32_t)dkv4::LDS_BYTES ? v->ldsBytes : (uint32_t)dkv4::LDS_BYTES;
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_dkv_p4<T, STREAM, false>);
  v->causal = v->own(&launch_dkv_p4<T, STREAM, true>);
  v->split = v->own(&launch_dkv_p4_split<T, STREAM>, 256);   // one workgroup per compute unit (512 registers per lane)
  v->splitCausal.splitTarget = 256;   // (the role-split kernel's pieces, as many as this kernel's)
}

// precision: Q, K, V and dO (one 16-bit type); lprec / dprec: storage types of L and D.  The streams exist for the two
// combinations the reference's descriptors produce (+Precisions.swift:13-96): FP16 L with BF16 D (mixed-precision mode)
// and FP32 L, D.  impl >= 1000 (developer build): stream index.
bool dkv16_p4_variant(int precision, int gprecision, int lprec, int dprec, int D, int impl, VariantInfo *out) {
  if (D != 128 && D != 64) return false;
  const bool mixed = lprec == PREC_FP16 && dprec == PREC_BF16, f32 = lprec == PREC_FP32 && dprec == PREC_FP32;
  const bool d64 = D == 64;
  if (precision == PREC_FP16 && gprecision == PREC_BF16) {   // the reference's own mix: FP16 Q, K, V with BF16 dO
    if (impl == 0 && mixed && !d64) { fill_dkv_p4<_Float16, dkv4::S_F16_DOBF16_MIXED>(out, "attn_dkv16p4_f16_dObf16_d128_w4x64"); return true; }
    if (impl == 0 && f32 && !d64) { fill_dkv_p4<_Float16, dkv4::S_F16_DOBF16_F32>(out, "attn_dkv16p4_f16_dObf16_d128_w4x64_exact"); return true; }
    if (impl == 0 && mixed && d64) { fill_dkv_p4<_Float16, dkv4::S_D64_F16_DOBF16_MIXED>(out, "attn_dkv16p4_f16_dObf16_d64_w4x64"); return true; }
    if (impl == 0 && f32 && d64) { fill_dkv_p4<_Float16, dkv4::S_D64_F16_DOBF16_F32>(out, "attn_dkv16p4_f16_dObf16_d64_w4x64_exact"); return true; }
    return false;
  }
  if (precision != gprecision) return false;
  if (precision == PREC_BF16) {
    if (impl == 0 && mixed && !d64) { fill_dkv_p4<__bf16, dkv4::S_BF16_MIXED>(out, "attn_dkv16p4_bf16_d128_w4x64"); return true; }
    if (impl == 0 && f32 && !d64) { fill_dkv_p4<__bf16, dkv4::S_BF16_F32>(out, "attn_dkv16p4_bf16_d128_w4x64_exact"); return true; }
    if (impl == 0 && mixed && d64) { fill_dkv_p4<__bf16, dkv4::S_D64_BF16_MIXED>(out, "attn_dkv16p4_bf16_d64_w4x64"); return true; }
    if (impl == 0 && f32 && d64) { fill_dkv_p4<__bf16, dkv4::S_D64_BF16_F32>(out, "attn_dkv16p4_bf16_d64_w4x64_exact"); return true; }
#ifdef MFA_DEV_VARIANTS
    if (impl == 1000 + dkv4::S_BF16_MIXED_PROF && mixed && !d64) { fill_dkv_p4<__bf16, dkv4::S_BF16_MIXED_PROF>(out, "attn_dkv16p4_DEV_BF16_MIXED_PROF"); return true; }
#endif
  }
  if (precision == PREC_FP16 && impl == 0) {
    if (mixed && !d64) { fill_dkv_p4<_Float16, dkv4::S_F16_MIXED>(out, "attn_dkv16p4_f16_d128_w4x64"); return true; }
    if (f32 && !d64) { fill_dkv_p4<_Float16, dkv4::S_F16_F32>(out, "attn_dkv16p4_f16_d128_w4x64_exact"); return true; }
    if (mixed && d64) { fill_dkv_p4<_Float16, dkv4::S_D64_F16_MIXED>(out, "attn_dkv16p4_f16_d64_w4x64"); return true; }
    if (f32 && d64) { fill_dkv_p4<_Float16, dkv4::S_D64_F16_F32>(out, "attn_dkv16p4_f16_d64_w4x64_exact"); return true; }
  }
  return false;
}

} // namespace mfa
