// attn_fwd16.hip -- instantiations of the 16-bit-MFMA forward kernel for gfx950.
#include "attn_fwd16.h"
#include "launchers.h"

namespace mfa {

template <typename T, int D, int NW, int RB>
static const char *launch_fwd16(const Launch &l) {
  // `l.grid` arrives as (row blocks, heads, batches); the kernel uses a flat XCD-aware order
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_fwd16<T, D, NW, RB>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          fwd16_lds_bytes<D>(), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, int RB>
static void fill(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * RB * 32;
  v->traversal = 64;
  v->headBlock = D;
  v->threads = NW * 64;
  v->ldsBytes = fwd16_lds_bytes<D>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_fwd16<T, D, NW, RB>);
}

// precision: PREC_FP16 or PREC_BF16; D: padded head dimension bucket
bool fwd16_variant(int precision, int D, VariantInfo *out) {
  if (precision == PREC_BF16) {
    switch (D) {
      case 32:  fill<__bf16, 32, 4, 1>(out, "attn_fwd16_bf16_d32_w4x32"); return true;
      case 64:  fill<__bf16, 64, 8, 1>(out, "attn_fwd16_bf16_d64_w8x32"); return true;
      case 128: fill<__bf16, 128, 8, 1>(out, "attn_fwd16_bf16_d128_w8x32"); return true;
      case 256: fill<__bf16, 256, 4, 1>(out, "attn_fwd16_bf16_d256_w4x32"); return true;
      default: return false;
    }
  }
  if (precision == PREC_FP16) {
    switch (D) {
      case 32:  fill<_Float16, 32, 4, 1>(out, "attn_fwd16_f16_d32_w4x32"); return true;
      case 64:  fill<_Float16, 64, 8, 1>(out, "attn_fwd16_f16_d64_w8x32"); return true;
      case 128: fill<_Float16, 128, 8, 1>(out, "attn_fwd16_f16_d128_w8x32"); return true;
      case 256: fill<_Float16, 256, 4, 1>(out, "attn_fwd16_f16_d256_w4x32"); return true;
      default: return false;
    }
  }
  return false;
}

} // namespace mfa
