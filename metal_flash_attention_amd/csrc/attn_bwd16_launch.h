// attn_bwd16_launch.h -- host-side launchers and VariantInfo fill templates of attn_bwd16.h
#pragma once
#include "attn_bwd16.h"
#include "launchers.h"
#include <cstdlib>

namespace mfa {


template <typename T, int D, int NW, typename TG = T>
static const char *launch_dq16(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dq16<T, D, NW, TG>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          (dq16_lds_bytes<D, NW>()), l.args, g);
  return nullptr;
}
template <typename T, int D, int NW, int PRE = 1, typename TG = T>
static const char *launch_dkv16(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dkv16<T, D, NW, PRE, TG>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          (dkv16_lds_bytes<D, NW>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, typename TG = T>
static const char *launch_dq16_causal(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dq16<T, D, NW, TG, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          (dq16_lds_bytes<D, NW>()), l.args, g);
  return nullptr;
}
template <typename T, int D, int NW, int PRE = 1, typename TG = T>
static const char *launch_dkv16_causal(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_dkv16<T, D, NW, PRE, TG, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          (dkv16_lds_bytes<D, NW>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, typename TG>
static const char *launch_dq16_sparse(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  if (l.args.causal)
    l.start(&attn_dq16<T, D, NW, TG, true, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64), (dq16_lds_bytes<D, NW>()), l.args, g);
  else
    l.start(&attn_dq16<T, D, NW, TG, false, true>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64), (dq16_lds_bytes<D, NW>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, typename TG>
static const char *launch_dq16_split(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, nullptr};
  const dim3 blocks(l.grid.x * l.grid.y * l.grid.z * l.splits);
  if (l.args.causal) l.start(&attn_dq16<T, D, NW, TG, true, false, true>, blocks, dim3(NW * 64), (dq16_lds_bytes<D, NW>()), l.args, g);
  else l.start(&attn_dq16<T, D, NW, TG, false, false, true>, blocks, dim3(NW * 64), (dq16_lds_bytes<D, NW>()), l.args, g);
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * l.args.R;
  l.start(&attn_bwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g, (int)SLOT_dQ, l.args.R, (const float *)l.wsO);
  return nullptr;
}

template <typename T, int D, int NW, typename TG = T>
static void fill_dq(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * 32;
  v->traversal = 64;
  v->headBlock = D;
  v->threads = NW * 64;
  v->ldsBytes = dq16_lds_bytes<D, NW>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_dq16<T, D, NW, TG>);
  v->causal = v->own(&launch_dq16_causal<T, D, NW, TG>);
  v->sparse = v->own(&launch_dq16_sparse<T, D, NW, TG>);
  v->split = v->splitCausal = v->own(&launch_dq16_split<T, D, NW, TG>);   // (the causal mask: a run-time flag of the pieces)
}
template <typename T, int D, int NW, int PRE = 1, typename TG = T>
static void fill_dkv(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * 32;
  v->traversal = 64;
  v->headBlock = D;
  v->threads = NW * 64;
  v->ldsBytes = dkv16_lds_bytes<D, NW>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_dkv16<T, D, NW, PRE, TG>);
  v->causal = v->own(&launch_dkv16_causal<T, D, NW, PRE, TG>);
}

// attn_dq16's buckets that have a translation unit each, behind dq16_variant (attn_bwd16.hip)
bool dq16_variant_d160(int precision, int gprecision, VariantInfo *out);
bool dq16_variant_d192(int precision, int gprecision, VariantInfo *out);

} // namespace mfa
