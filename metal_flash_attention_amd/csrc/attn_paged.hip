// attn_paged.hip -- instantiations of the any-head-dimension kernels (attn_paged.h): D-blocked products, accumulators paged
// through the output buffers (the reference's scheme beyond what registers hold, +Accumulate.swift:403-469).
#include "attn_paged.h"
#include "launchers.h"

namespace mfa {

template <void (*KERNEL)(const KernelArgs, const paged::Grid)>
static const char *launch_paged(const Launch &l) {
  paged::Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(KERNEL, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(256), 0, l.args, g);
  return nullptr;
}

template <void (*KERNEL)(const KernelArgs, const paged::Grid)> static void fill_paged(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = paged::BR;   // rows (forward, backwardQuery) or keys (backwardKeyValue) per workgroup
  v->traversal = paged::BC;
  v->headBlock = paged::DC;         // the head dimension is walked in chunks of 64, whatever D is
  v->threads = 256;
  v->ldsBytes = 0;                  // static LDS only
  v->cacheLeft = false;             // nothing is cached: every operand block is re-staged per traversal step
  v->cacheSecond = false;
  v->pagedAccumulators = true;
  // causal mask, per-batch lengths and block masks are handled by the one code object
  v->dense = v->causal = v->sparse = v->own(&launch_paged<KERNEL>);
}

bool paged_variant(int type, VariantInfo *out) {
  switch (type) {
    case 0: fill_paged<attn_paged_fwd>(out, "attn_paged_fwd_f32_any_d"); return true;
    case 1: fill_paged<attn_paged_dq>(out, "attn_paged_dq_f32_any_d"); return true;
    case 2: fill_paged<attn_paged_dkv>(out, "attn_paged_dkv_f32_any_d"); return true;
    default: return false;
  }
}

} // namespace mfa
