// attn_dkv16_rs_launch.h -- host-side launchers and VariantInfo fill templates of attn_dkv16_rs.h
#pragma once
#include "attn_dkv16_rs.h"
#include "launchers.h"

namespace mfa {


template <typename T, int D, typename TG, bool CAUSAL, int ABL = 0>
static const char *launch_rs(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dkv16_rs<T, D, TG, CAUSAL, ABL>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(dkv16rs_pairs<D>() * 128), (dkv16rs_lds_bytes<D>()),
          l.args, g);
  return nullptr;
}

template <typename T, int D, typename TG>
static const char *launch_rs_sparse(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  if (l.args.causal)
    l.start(&attn_dkv16_rs<T, D, TG, true, 0, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(dkv16rs_pairs<D>() * 128), (dkv16rs_lds_bytes<D>()), l.args, g);
  else
    l.start(&attn_dkv16_rs<T, D, TG, false, 0, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(dkv16rs_pairs<D>() * 128), (dkv16rs_lds_bytes<D>()), l.args, g);
  return nullptr;
}

template <typename T, int D, typename TG>
static const char *launch_rs_split(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, nullptr};
  const dim3 blocks(l.grid.x * l.grid.y * l.grid.z * l.splits), threads(dkv16rs_pairs<D>() * 128);
  if (l.args.causal) l.start(&attn_dkv16_rs<T, D, TG, true, 0, false, true>, blocks, threads, (dkv16rs_lds_bytes<D>()), l.args, g);
  else l.start(&attn_dkv16_rs<T, D, TG, false, 0, false, true>, blocks, threads, (dkv16rs_lds_bytes<D>()), l.args, g);
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * l.args.C;
  const float *dk_slabs = l.wsO + (uint64_t)l.splits * rows * l.args.D;   // dV slabs first, then dK slabs
  l.start(&attn_bwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g, (int)SLOT_dV, l.args.C, (const float *)l.wsO);
  l.start(&attn_bwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g, (int)SLOT_dK, l.args.C, dk_slabs);
  return nullptr;
}

template <typename T, int D, typename TG = T>
static void fill(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = dkv16rs_pairs<D>() * 32;   // key columns per workgroup: wave pairs x 32
  v->traversal = 32;
  v->headBlock = D;
  v->threads = dkv16rs_pairs<D>() * 128;
  v->ldsBytes = dkv16rs_lds_bytes<D>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_rs<T, D, TG, false>);
  v->causal = v->own(&launch_rs<T, D, TG, true>);
  v->sparse = v->own(&launch_rs_sparse<T, D, TG>);
  v->split = v->splitCausal = v->own(&launch_rs_split<T, D, TG>);   // (the causal mask: a run-time flag of the pieces)
}

// the family's buckets that have a translation unit each, behind dkv16_rs_variant (attn_dkv16_rs.hip)
bool dkv16_rs_variant_d96(int precision, int gprecision, VariantInfo *out);
bool dkv16_rs_variant_d160(int precision, int gprecision, VariantInfo *out);
bool dkv16_rs_variant_d192(int precision, int gprecision, VariantInfo *out);

} // namespace mfa
