// attn_fwd16_v3_launch.h -- host-side launchers and VariantInfo fill templates of attn_fwd16_v3.h (shared by attn_fwd16_v3.hip and the per-head-dimension bucket TUs)
#pragma once
#include "attn_fwd16_v3.h"
#include "launchers.h"

namespace mfa {


// LDS bytes of a schedule: the LDS-DMA schedule on the 2-stage ring keeps three K and two V images (all 160 KiB)
template <int D, int NW, int RB, int RING, int VD> constexpr int fwd16v3_lds_bytes() {
  if ((VD & 32) && RING == 2) return 5 * 64 * D * 2;
  return fwd16v2_lds_bytes<D, NW, RB, RING, (VD & 2) ? 16 : 0>();
}

template <typename T, int D, int NW, int RB, int THR, int PRE, int ABL = 0, int RING = 3, int VD = 0>
static const char *launch_v3(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_fwd16_v3<T, D, NW, RB, THR, PRE, ABL, RING, false, false, VD>, dim3(l.grid.x * l.grid.y * l.grid.z), dim3(NW * 64),
          (fwd16v3_lds_bytes<D, NW, RB, RING, VD>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, int RB, int THR, int PRE, int ABL = 0, int RING = 3, int VD = 0>
static const char *launch_v3_split(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z, l.splits, l.wsO, l.wsML};
  l.start(&attn_fwd16_v3<T, D, NW, RB, THR, PRE, ABL, RING, true, false, VD>, dim3(l.grid.x * l.grid.y * l.grid.z * l.splits),
          dim3(NW * 64), (fwd16v3_lds_bytes<D, NW, RB, RING, VD>()), l.args, g);
  const uint64_t rows = (uint64_t)l.grid.y * l.grid.z * l.args.R;
  l.start(&attn_fwd_combine, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, int RB, int THR, int PRE, int ABL = 0, int RING = 3, int VD = 0>
static void fill(VariantInfo *v, const char *name) {
  v->name = name;
  v->parallelization = NW * RB * 32;
  v->traversal = 32;   // pipeline step: half a 64-key LDS tile (attn_fwd16_v3.h)
  v->headBlock = D;
  v->threads = NW * 64;
  v->ldsBytes = fwd16v3_lds_bytes<D, NW, RB, RING, VD>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->dense = v->own(&launch_v3<T, D, NW, RB, THR, PRE, ABL, RING, VD>);
}

template <typename T, int D, int NW, int RB, int THR, int PRE, int RING, int VD>
static const char *launch_v3_causal(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_fwd16_v3<T, D, NW, RB, THR, PRE, 0, RING, false, true, VD>, dim3(l.grid.x * l.grid.y * l.grid.z),
          dim3(NW * 64), (fwd16v3_lds_bytes<D, NW, RB, RING, VD>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, int RB, int THR, int PRE, int RING, int VD>
static const char *launch_v3_sparse(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  if (l.args.causal)
    l.start(&attn_fwd16_v3<T, D, NW, RB, THR, PRE, 0, RING, false, true, VD, true>, dim3(l.grid.x * l.grid.y * l.grid.z),
            dim3(NW * 64), (fwd16v3_lds_bytes<D, NW, RB, RING, VD>()), l.args, g);
  else
    l.start(&attn_fwd16_v3<T, D, NW, RB, THR, PRE, 0, RING, false, false, VD, true>, dim3(l.grid.x * l.grid.y * l.grid.z),
            dim3(NW * 64), (fwd16v3_lds_bytes<D, NW, RB, RING, VD>()), l.args, g);
  return nullptr;
}

// product variants: the dense code object plus its causal, block-sparse and column-parallel siblings (VDS: schedule
// bits of the block-sparse pair, which restarts its pipeline per run of active tiles and keeps register staging)
template <typename T, int D, int NW, int RB, int THR, int PRE, int RING = 3, int VD = 0, int PRES = PRE, int VDS = VD>
static void fill_with_split(VariantInfo *v, const char *name) {
  fill<T, D, NW, RB, THR, PRE, 0, RING, VD>(v, name);
  v->sparse = v->own(&launch_v3_sparse<T, D, NW, RB, THR, PRES, RING, VDS>);
  v->split = v->own(&launch_v3_split<T, D, NW, RB, THR, PRE, 0, RING, VD>);
  v->causal = v->own(&launch_v3_causal<T, D, NW, RB, THR, PRE, RING, VD>);
}

// transposed operands read in place (TR of attn_fwd16_v3.h): one code object per pattern of (K, V); Q / O and the causal mask
// are run-time flags of these kernels.  No column-parallel or block-sparse siblings: such launches stay row-parallel /
// go to the general kernel.
template <typename T, int D, int NW, int RING, int VD, int TR>
static const char *launch_v3_tr(const Launch &l) {
  Fwd16Grid g{l.grid.x, l.grid.y, l.grid.z};
  l.start(&attn_fwd16_v3<T, D, NW, 1, 8, 0, 0, RING, false, true, VD, false, TR>, dim3(l.grid.x * l.grid.y * l.grid.z),
          dim3(NW * 64), (fwd16v3_lds_bytes<D, NW, 1, RING, VD>()), l.args, g);
  return nullptr;
}

template <typename T, int D, int NW, int RING, int VD, int TR>
static void fill_tr(VariantInfo *v, const char *name) {
  *v = VariantInfo();
  v->name = name;
  v->parallelization = NW * 32;
  v->traversal = 32;
  v->headBlock = D;
  v->threads = NW * 64;
  v->ldsBytes = fwd16v3_lds_bytes<D, NW, 1, RING, VD>();
  v->cacheLeft = true;
  v->cacheSecond = true;
  v->transposedInPlace = true;
  v->dense = v->causal = v->own(&launch_v3_tr<T, D, NW, RING, VD, TR>);   // (the causal mask: a run-time flag)
}

// pattern: bit 0 = K transposed, bit 1 = V transposed (Q / O: any)
#define MFA_FWD16_V3_TR_BUCKET(T, TNAME, D, NW, RING, VD, GEOM)                                                                   \
  switch (pattern) {                                                                                                               \
    case 0: fill_tr<T, D, NW, RING, VD, 4>(out, "attn_fwd16v3_" TNAME "_d" #D "_" GEOM "_thr8_tr"); return true;                 \
    case 1: fill_tr<T, D, NW, RING, VD, 5>(out, "attn_fwd16v3_" TNAME "_d" #D "_" GEOM "_thr8_tr_k"); return true;               \
    case 2: fill_tr<T, D, NW, RING, VD, 6>(out, "attn_fwd16v3_" TNAME "_d" #D "_" GEOM "_thr8_tr_v"); return true;               \
    case 3: fill_tr<T, D, NW, RING, VD, 7>(out, "attn_fwd16v3_" TNAME "_d" #D "_" GEOM "_thr8_tr_kv"); return true;              \
    default: return false;                                                                                                         \
  }

// the family's buckets that have a translation unit each, behind fwd16_v3_variant / fwd16_v3_tr_variant (attn_fwd16_v3.hip)
bool fwd16_v3_variant_d160(int precision, VariantInfo *out);
bool fwd16_v3_variant_d192(int precision, VariantInfo *out);
bool fwd16_v3_tr_variant_d64(int precision, int D, int pattern, VariantInfo *out);   // buckets 32, 64
bool fwd16_v3_tr_variant_d128(int precision, int D, int pattern, VariantInfo *out);
bool fwd16_v3_tr_variant_d160(int precision, int D, int pattern, VariantInfo *out);
bool fwd16_v3_tr_variant_d192(int precision, int D, int pattern, VariantInfo *out);
bool fwd16_v3_tr_variant_d256(int precision, int D, int pattern, VariantInfo *out);

} // namespace mfa
