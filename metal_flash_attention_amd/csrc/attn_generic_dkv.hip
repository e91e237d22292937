// attn_generic_dkv.hip -- instantiations of the generic (fp32-MFMA) dkv kernel for gfx950.
#include "attn_generic.h"
#include "launchers.h"
#include <cstdlib>

namespace mfa {

template <int DP, int NW, bool CACHE, bool X = false>
static const char *launch_dkv(const Launch &l) {
  constexpr uint32_t lds = generic_dkv_lds_floats<DP, NW, CACHE, X>() * sizeof(float);
  l.start(&attn_generic_dkv<DP, NW, CACHE, false, X>, l.grid, dim3(NW * 64), lds, l.args);
  return nullptr;
}

template <int DP, int NW, bool CACHE, bool X = false>
static const char *launch_dkv_masked(const Launch &l) {
  constexpr uint32_t lds = generic_dkv_lds_floats<DP, NW, CACHE, X>() * sizeof(float);
  l.start(&attn_generic_dkv<DP, NW, CACHE, true, X>, l.grid, dim3(NW * 64), lds, l.args);
  return nullptr;
}

template <int DP, int NW, bool CACHE, bool X = false>
static void fill(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * 32;
  v->traversal = 32;
  v->headBlock = DP;
  v->threads = NW * 64;
  v->ldsBytes = generic_dkv_lds_floats<DP, NW, CACHE, X>() * sizeof(float);
  v->cacheLeft = CACHE;
  v->cacheSecond = CACHE;
  v->sparse = v->own(&launch_dkv_masked<DP, NW, CACHE, X>);       // block mask: own code objects
  v->dense = v->causal = v->own(&launch_dkv<DP, NW, CACHE, X>);   // (the causal mask: a run-time flag)
}

bool generic_dkv_variant(int DP, VariantInfo *out) {
  switch (DP) {
    case 32:  fill<32, 4, true>(out, "attn_generic_dkv_f32mfma_d32_w4_cached"); return true;
    case 64:  fill<64, 4, true>(out, "attn_generic_dkv_f32mfma_d64_w4_cached"); return true;
    case 128: fill<128, 4, true>(out, "attn_generic_dkv_f32mfma_d128_w4_cached"); return true;   // (2 waves per workgroup, i.e. half the LDS and twice the workgroups per CU: 10-15 % slower, measured)
    case 256: fill<256, 4, true>(out, "attn_generic_dkv_f32mfma_d256_w4_cached"); return true;
    case 384: fill<384, 1, false, true>(out, "attn_generic_dkv_f32mfma_d384_w1_streamed"); return true;
    default: return false;
  }
}

} // namespace mfa
