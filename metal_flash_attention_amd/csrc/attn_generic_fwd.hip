// attn_generic_fwd.hip -- instantiations of the generic (fp32-MFMA) fwd kernel for gfx950.
#include "attn_generic.h"
#include "launchers.h"
#include <cstdlib>

namespace mfa {

template <int DP, int NW, bool CACHE>
static const char *launch_fwd(const Launch &l) {
  constexpr uint32_t lds = generic_fwd_lds_floats<DP, NW, CACHE>() * sizeof(float);
  l.start(&attn_generic_fwd<DP, NW, CACHE>, l.grid, dim3(NW * 64), lds, l.args);
  return nullptr;
}

template <int DP, int NW, bool CACHE>
static const char *launch_fwd_masked(const Launch &l) {
  constexpr uint32_t lds = generic_fwd_lds_floats<DP, NW, CACHE>() * sizeof(float);
  l.start(&attn_generic_fwd<DP, NW, CACHE, true>, l.grid, dim3(NW * 64), lds, l.args);
  return nullptr;
}

template <int DP, int NW, bool CACHE>
static void fill(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * 32;
  v->traversal = 32;
  v->headBlock = DP;
  v->threads = NW * 64;
  v->ldsBytes = generic_fwd_lds_floats<DP, NW, CACHE>() * sizeof(float);
  v->cacheLeft = CACHE;
  v->cacheSecond = CACHE;
  v->sparse = v->own(&launch_fwd_masked<DP, NW, CACHE>);       // block mask: own code objects
  v->dense = v->causal = v->own(&launch_fwd<DP, NW, CACHE>);   // (the causal mask: a run-time flag)
}

bool generic_fwd_variant(int DP, VariantInfo *out) {
  switch (DP) {
    case 32:  fill<32, 4, true>(out, "attn_generic_fwd_f32mfma_d32_w4_cached"); return true;
    case 64:  fill<64, 4, true>(out, "attn_generic_fwd_f32mfma_d64_w4_cached"); return true;
    case 128: fill<128, 4, true>(out, "attn_generic_fwd_f32mfma_d128_w4_cached"); return true;   // (2 waves per workgroup, i.e. half the LDS and twice the workgroups per CU: 10-15 % slower, measured)
    case 256: fill<256, 4, true>(out, "attn_generic_fwd_f32mfma_d256_w4_cached"); return true;
    // D <= 384: two waves per workgroup (64 rows x 385 floats of LDS staging), 192 registers of O and 192 of Q per lane
    case 384: fill<384, 2, true>(out, "attn_generic_fwd_f32mfma_d384_w2_cached"); return true;
    default: return false;
  }
}

} // namespace mfa
