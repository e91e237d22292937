// launchers.h -- host-side entry points of each kernel translation unit (internal, C++).
#pragma once
#include "attn_common.h"

namespace mfa {

// Every attention launch goes through launch_kernel: a kernel that takes more than 64 KiB of dynamic LDS has that limit raised the
// first time it is launched on a device (raise_lds_limit, mfa_kernel.hip); after that a launch makes no driver call but the launch
// itself, which is what graph capture needs.  A failure to raise the limit launches nothing and is returned.
hipError_t raise_lds_limit(const void *kernel, uint32_t bytes);
template <typename... Params, typename... Args>
hipError_t launch_kernel(void (*kernel)(Params...), dim3 grid, dim3 block, uint32_t lds, hipStream_t stream, const Args &...args) {
  if (lds > 64 * 1024) {
    const hipError_t err = raise_lds_limit(reinterpret_cast<const void *>(kernel), lds);
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  return hipSuccess;
}

// One launch as an entry point of a variant sees it.  The entry point decides which code object serves the launch, starts it when
// `run` is set, and returns the launch form's text for that choice (mfa_attention_kernel_launch_form): nullptr = the code object of
// the variant that owns the route (Route::owner).  The same entry point answers mfa_attention_kernel_launch / _time (run) and
// _launch_form (not run), so what runs is what the form names.  `grid` counts the route's workgroups (Route::parallelization); an
// entry point that starts a kernel of another workgroup size derives that kernel's block count from `args`.
struct Launch {
  const KernelArgs &args;
  dim3 grid;
  uint32_t splits;         // > 1: column-parallel pieces, partial results in wsO (and wsML: forward)
  float *wsO, *wsML;
  hipStream_t stream;
  bool run;
  mutable hipError_t err;  // the first failed HIP call of a run; nothing is started after it
  template <typename... Params, typename... Args>
  void start(void (*kernel)(Params...), dim3 g, dim3 block, uint32_t lds, const Args &...a) const {
    if (run && err == hipSuccess) err = launch_kernel(kernel, g, block, lds, stream, a...);
  }
};
typedef const char *(*LaunchFn)(const Launch &l);

// compute units of the current device (mfa_kernel.hip; cached per device)
hipError_t compute_units(int *cus);

// How a variant serves one kind of launch: the entry point, the rows (fwd, dQ) or columns (dK/dV) per workgroup of the kernel it
// starts, and the variant the route belongs to.  A hand-placed variant laid over a compiler-scheduled one arrives filled by it and
// overwrites only the routes it serves; the others keep their owner, who the launch form then names.  An empty route: the variant
// does not serve that kind of launch (the general kernel does; split routes: the launch is not split).
struct Route {
  LaunchFn launch = nullptr;
  uint16_t parallelization = 0;
  uint16_t splitTarget = 0;     // split routes: workgroups the pieces aim at (0: 512 = two per compute unit)
  const char *owner = nullptr;
  explicit operator bool() const { return launch != nullptr; }
};

struct VariantInfo {
  const char *name = "";
  uint16_t parallelization = 0; // rows (fwd, dQ) or columns (dK/dV) per workgroup
  uint16_t traversal = 0;       // columns (fwd, dQ) or rows (dK/dV) per main-loop step
  uint16_t headBlock = 0;       // padded head dimension the code object is unrolled for
  uint32_t threads = 0;         // work-items per workgroup
  uint32_t ldsBytes = 0;        // dynamic LDS of the variant's code object (mfa_attention_kernel_threadgroup_memory_allocation)
  bool cacheLeft = false;       // left-hand operands cached in VGPRs (Q / Q,dO / K,V)
  bool cacheSecond = false;     // the second of them alone (dO / V); fill code sets it = cacheLeft unless a variant splits the pair
  bool pagedAccumulators = false;   // accumulators paged through the output buffers (any-D kernels, attn_paged.h); else in registers
  bool transposedInPlace = false;   // reads / writes transposed operands where they lie, whatever their alignment (attn_fwd16_v3.h, TR)
  // one route per kind of launch.  A code object that takes the causal flag or the block mask itself serves those routes with its
  // dense entry point.  Forward split entry points take no causal flag: forward splitCausal stays empty
  Route dense, causal, sparse, split, splitCausal;
  // a route of this variant's own kernel (name and parallelization as set)
  Route own(LaunchFn f, uint16_t splitTarget = 0) const { return {f, parallelization, splitTarget, name}; }
  // the route of a launch: pieces of a column-parallel launch, a block mask, the causal mask or none
  const Route &route(bool pieces, bool masked, bool isCausal) const {
    if (pieces) return isCausal ? splitCausal : split;
    if (masked) return sparse;
    return isCausal ? causal : dense;
  }
};

// any head dimension (D > 384): D-blocked products, accumulators paged through the FP32 output buffers (attn_paged.h); type = kernel type
bool paged_variant(int type, VariantInfo *out);

// generic (fp32-MFMA) family: returns false if (DP) is not compiled
// FP32 descriptors with row-major operands and D % 4 == 0 at the 64 / 128 head blocks: the variant IS the FP32 production kernel
// (own name, own LDS bytes); `out` arrives filled by generic_*_variant(DP), whose kernel becomes the sibling that keeps block-sparse
// launches and launches whose operands miss the 16-byte row alignment.  The FP32 kernels take the launches whose operands qualify
// (all FP32, row-major, 16-byte aligned rows, D % 4 == 0, no block mask).  type: 0 forward, 1 backwardQuery, 2 backwardKeyValue
bool f32_variant(int type, int DP, VariantInfo *out);
bool generic_fwd_variant(int DP, VariantInfo *out);
bool generic_dq_variant(int DP, VariantInfo *out);
bool generic_dkv_variant(int DP, VariantInfo *out);

// 16-bit MFMA forward family (Q, K, V in one 16-bit type, row-major, D % 8 == 0)
bool fwd16_variant(int precision, int D, VariantInfo *out);
// software-pipelined version; impl selects an experimental schedule (see attn_fwd16_v2.hip)
bool fwd16_v2_variant(int precision, int D, int impl, VariantInfo *out);
// one wave per SIMD, 64 query rows per wave, half-tile pipeline (see attn_fwd16_v3.h); D = the head-dimension bucket: 32, 64, 128, 256
// (attn_fwd16_v3.hip) and 160, 192 (a translation unit each).  Like every family entry: false = no code object for these arguments
bool fwd16_v3_variant(int precision, int D, int impl, VariantInfo *out);
// operands stored transposed, read in place (TR kernels of attn_fwd16_v3.h): pattern bit 0 = K, bit 1 = V transposed (Q / O: any);
// buckets 32 .. 256
bool fwd16_v3_tr_variant(int precision, int D, int pattern, VariantInfo *out);
// four waves x 64 rows, one wave per SIMD, hand-placed instruction stream (attn_fwd16_p4.h); D <= 128 only
bool fwd16_p4_variant(int precision, int D, int impl, VariantInfo *out);
// D <= 64: four waves x 64 rows, persistent (attn_fwd16_p6.h; fold = the descriptor holds the attention matrix in 16-bit registers:
// scale folded into Q, row sums in the matrix pipe); `out` arrives filled by fwd16_v3_variant(precision, 64, 0), whose kernel keeps
// the launches this one does not serve
bool fwd16_p6_variant(int precision, bool fold, VariantInfo *out);
// 256 < D <= 384 (head blocks 320, 384): four waves x 32 rows, 32-key steps, compiler-scheduled (attn_fwd16_wide.h, round 6)
bool fwd16_wide_variant(int precision, int D, VariantInfo *out);
// the backward kernels of the same head blocks (attn_bwd16_wide.hip: attn_dq16 with 32-key tiles, attn_dkv16_wide.h; round 6)
bool dq16_wide_variant(int precision, int gprecision, int D, VariantInfo *out);
bool dkv16_wide_variant(int precision, int gprecision, int D, VariantInfo *out);
// 128 < D <= 256: four waves x 64 rows, 32-key steps (attn_fwd16_p5.h); `out` arrives filled by fwd16_v3_variant
bool fwd16_p5_variant(int precision, int D, int impl, VariantInfo *out);
// backwardKeyValue counterpart: four waves x 64 keys (attn_dkv16_p4.h); `out` arrives filled by dkv16_rs_variant, whose
// split / block-sparse launchers it keeps.  lprec / dprec: storage types of L and D (fixed per instruction stream)
bool dkv16_p4_variant(int precision, int gprecision, int lprec, int dprec, int D, int impl, VariantInfo *out);
// buckets 160 / 192 / 256: role-split wave pairs x 64 keys, hand-placed stream (attn_dkv16_p5.h); `out` arrives filled by the 32-key
// role-split kernel of the bucket (attn_dkv16_rs.h), which keeps the block-sparse and row-parallel launches
bool dkv16_p5_variant(int precision, int gprecision, int lprec, int dprec, int D, VariantInfo *out);
// buckets 160 / 192 / 256: role-split wave pairs x 64 rows, hand-placed stream (attn_dq16_p5.h); `out` arrives filled by the 32-row-wave
// kernel of the bucket (attn_bwd16.h attn_dq16), which keeps the block-sparse and column-parallel launches
bool dq16_p5_variant(int precision, int gprecision, int D, int impl, VariantInfo *out);
// backwardQuery counterpart: four waves x 64 rows (attn_dq16_p4.h); `out` arrives filled by dq16_variant
bool dq16_p4_variant(int precision, int gprecision, int D, int impl, VariantInfo *out);
// 8 waves x 32 rows, SIMD partners alternate matrix / vector segments (see attn_fwd16_v4.h)
bool fwd16_v4_variant(int precision, int D, int impl, VariantInfo *out);

// 16-bit MFMA backward kernels (Q, K, V, dO in one 16-bit type, row-major; gprecision = storage type of dO: the same 16-bit type,
// or BF16 next to FP16 Q/K/V).  D = the head-dimension bucket: dQ 64, 128, 160, 192, 256; dK/dV one wave per key block 64, 128
bool dq16_variant(int precision, int gprecision, int D, VariantInfo *out);
bool dkv16_variant(int precision, int gprecision, int D, VariantInfo *out);
// role-split wave pairs: one wave of a SIMD accumulates dV, its partner dK (see attn_dkv16_rs.h); buckets 64, 96, 128, 160, 192, 256.
// The buckets 160 / 192 of the trio and 96 of this kernel have a translation unit each.  Measured at N = 4096, 64 heads
// (profiles/r02_bucket_perf.txt): the 96-wide forward and dQ objects LOSE to the 128 objects run on zero-padded chunks (0.576 vs
// 0.499 ms, 0.885 vs 0.781 ms) and are not built; dK/dV wins at 96 (1.02 vs 1.18 ms)
bool dkv16_rs_variant(int precision, int gprecision, int D, int impl, VariantInfo *out);

// K and / or V transposed at D <= 128 (pattern: bit 0 = K, bit 1 = V): launches of whole chunks of aligned rows run the hand-placed
// stream (attn_fwd16_p4_tr.h); `out` arrives filled by fwd16_v3_tr_variant at bucket 128, whose kernel keeps the others
bool fwd16_p4_tr_variant(int precision, int pattern, bool fold, VariantInfo *out);

// backward kernels that read transposed operands in place (attn_bwd16_p4_tr.hip; l.grid = (row or column blocks, heads, batches)):
// the launch form's text, nullptr = not a launch these kernels take (nothing is started then)
const char *bwd16_p4_tr_launch(int type, bool fold, const Launch &l);
// launches with K^T and / or V^T at the buckets 160 / 192 / 256 that are whole 32-key steps of aligned rows go
// to the hand-placed stream (attn_fwd16_p5_tr.h); `out` arrives filled by fwd16_v3_tr_variant of the bucket, whose kernel keeps the others
bool fwd16_p5_tr_variant(int precision, int bucket, int pattern, bool fold, VariantInfo *out);

// grouped-query backwardKeyValue (attn_kv_group_sum.hip): dK / dV head j = sum over g < G, in order, of the fp32 slabs
// [batch][query head][column][D] of query heads jG + g, stored through the caller's views `dv` / `dk` (whose strides count K / V heads)
hipError_t launch_kv_group_sum(const float *dvSlabs, const float *dkSlabs, const OperandView &dv, const OperandView &dk, uint32_t G,
                               uint32_t kvHeads, uint32_t batches, uint32_t C, uint32_t D, const uint32_t *colLen, hipStream_t stream);

} // namespace mfa
