// mfa_kernel.hip -- AttentionKernel object and launch planning (C ABI of include/mfa.h); which code object a descriptor selects:
// variant_select.cpp.
//
// Replaces, for gfx950, the Metal calls the reference's callers make around an AttentionKernel (Sources/FlashAttention/Attention/
// AttentionKernel/AttentionKernel.swift:268-363; Tests/FlashAttentionTests/Attention/SquareAttentionTest.swift:244-260, :319-368).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <utility>

#include "cache_launch.h"
#include "launchers.h"
#include "mfa_internal.h"
#include "variant_select.h"

using namespace mfa;

struct mfa_attention_kernel {
  mfa_attention_kernel_descriptor desc;  // as requested
  mfa_attention_kernel_descriptor effective; // what the selected code object really does
  VariantInfo variant;            // preferred code object
  VariantInfo fallback;           // general code object, used when a launch does not meet the
  bool hasFallback = false;       // preferred variant's alignment requirements
  bool relayout = false;          // transposed operands: the preferred variant runs on row-major copies in the caller's workspace
};

// launch_kernel (launchers.h): the dynamic-LDS limit of a code object, raised once per (kernel, device)
hipError_t mfa::raise_lds_limit(const void *kernel, uint32_t bytes) {
  static std::mutex guard;
  static std::set<std::pair<const void *, int>> raised;
  int device = 0;
  hipError_t err = hipGetDevice(&device);
  if (err != hipSuccess) return err;
  const std::pair<const void *, int> key(kernel, device);
  std::lock_guard<std::mutex> lock(guard);
  if (raised.count(key)) return hipSuccess;
  err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (err == hipSuccess) raised.insert(key);
  return err;
}

// the persistent launchers (attn_fwd16_p4p.hip, attn_fwd16_p6.hip): compute units of the current device, cached per device
hipError_t mfa::compute_units(int *cus) {
  static std::mutex guard;
  static int cached[64] = {};
  int device = 0;
  hipError_t err = hipGetDevice(&device);
  if (err != hipSuccess) return err;
  const bool cache = device >= 0 && device < 64;
  std::lock_guard<std::mutex> lock(guard);
  if (cache && cached[device] > 0) { *cus = cached[device]; return hipSuccess; }
  err = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device);
  if (err == hipSuccess && *cus <= 0) err = hipErrorInvalidValue;
  if (err == hipSuccess && cache) cached[device] = *cus;
  return err;
}

extern "C" {

// AttentionKernel.init guard (AttentionKernel.swift:28-34) and what the kernel type needs to know of each operand it touches
static mfa_status check_descriptor(const mfa_attention_kernel_descriptor *kdesc) {
  if (!kdesc->hasBlockDimensions || !kdesc->hasHeadDimension || kdesc->preferAsyncCache < 0 ||
      kdesc->preferAsyncLoad < 0 || kdesc->type < 0)
    return fail(MFA_ERR_INCOMPLETE_DESCRIPTOR, "Descriptor was incomplete.");
  const int type = kdesc->type;
  if (type > 2) return fail(MFA_ERR_INVALID_ARGUMENT, "unknown kernel type");
  if (kdesc->headDimension == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "headDimension must be non-zero");
  for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot) {
    if (!slot_used(type, slot)) continue;
    const int op = slot_operand(slot);
    const int prec = kdesc->memoryPrecisions[op];
    if (prec < 0)  // AttentionKernel.swift:56-58 "Memory precision of X was not specified."
      return fail(MFA_ERR_INCOMPLETE_DESCRIPTOR, std::string("Memory precision of ") + mfa_operand_name(op) + " was not specified.");
    if (prec > MFA_BF16) return fail(MFA_ERR_INVALID_ARGUMENT, "unknown precision");
    if (op != MFA_L && op != MFA_D && kdesc->transposeState[op] < 0)
      return fail(MFA_ERR_INCOMPLETE_DESCRIPTOR, std::string("Transpose state of ") + mfa_operand_name(op) + " was not specified.");
  }
  return MFA_OK;
}

// instead of emitting shader source for a JIT, the descriptor selects one of the pre-compiled code objects (variant_select.cpp)
mfa_status mfa_attention_kernel_create(const mfa_attention_kernel_descriptor *kdesc, mfa_attention_kernel **out) {
  if (!kdesc || !out) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  mfa_status st = check_descriptor(kdesc);
  if (st != MFA_OK) return st;
  Selection selected;
  st = select_variant(*kdesc, &selected);
  if (st != MFA_OK) return st;
  mfa_attention_kernel *kernel = new mfa_attention_kernel();
  kernel->desc = *kdesc;
  kernel->effective = selected.effective;
  kernel->variant = selected.variant;
  kernel->fallback = selected.general;
  kernel->hasFallback = selected.fast;
  kernel->relayout = selected.relayout;
  *out = kernel;
  return MFA_OK;
}

void mfa_attention_kernel_destroy(mfa_attention_kernel *kernel) { delete kernel; }

mfa_status mfa_attention_kernel_block_dimensions(const mfa_attention_kernel *kernel, uint16_t *parallelization,
                                                 uint16_t *traversal, uint16_t *headBlock) {
  if (!kernel) return fail(MFA_ERR_INVALID_ARGUMENT, "null kernel");
  if (parallelization) *parallelization = kernel->variant.parallelization;
  if (traversal) *traversal = kernel->variant.traversal;
  if (headBlock) *headBlock = kernel->variant.headBlock;
  return MFA_OK;
}

uint32_t mfa_attention_kernel_threadgroup_size(const mfa_attention_kernel *kernel) {
  return kernel ? kernel->variant.threads : 0;
}
uint32_t mfa_attention_kernel_threadgroup_memory_allocation(const mfa_attention_kernel *kernel) {
  return kernel ? kernel->variant.ldsBytes : 0;
}
const char *mfa_attention_kernel_variant(const mfa_attention_kernel *kernel) {
  return kernel ? kernel->variant.name : "";
}
const char *mfa_attention_kernel_fallback_variant(const mfa_attention_kernel *kernel) {
  return kernel && kernel->hasFallback ? kernel->fallback.name : "";
}
int mfa_attention_kernel_needs_workspace_for_fast_path(const mfa_attention_kernel *kernel) {
  return kernel && kernel->relayout ? 1 : 0;
}
mfa_status mfa_attention_kernel_effective_descriptor(const mfa_attention_kernel *kernel,
                                                     mfa_attention_kernel_descriptor *out) {
  if (!kernel || !out) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  *out = kernel->effective;
  return MFA_OK;
}

// true if this launch satisfies the 16-byte-chunk requirements of the 16-bit MFMA kernels
static bool meets_fast_requirements(const mfa_attention_kernel *kernel, const KernelArgs &args) {
  const int type = kernel->desc.type;
  for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot) {
    if (!slot_used(type, slot) || slot == SLOT_L || slot == SLOT_D) continue;
    const OperandView &v = args.op[slot];
    const int64_t per16 = 16 / (v.precision == PREC_FP32 ? 4 : 2);  // elements per 16 bytes
    // (transposed views: the kernels that read them in place gather what is not 16-byte aligned)
    const bool anyAlignment = v.transposed && kernel->variant.transposedInPlace;
    if (!anyAlignment && (reinterpret_cast<uintptr_t>(v.ptr) & 15) != 0) return false;
    if (!anyAlignment && (v.ld % per16 || v.headStride % per16 || v.batchStride % per16)) return false;
    // these kernels address one (head, batch) slice through a buffer descriptor with 32-bit byte
    // offsets (prefetch may run two tiles past the end): larger slices use the general kernels
    const uint64_t seq = row_operand(slot_operand(slot)) ? args.R : args.C;
    // (transposed views, forward only: D rows of `ld` elements; the prefetch runs two tiles = 128 elements along the last row)
    const uint64_t bytes = (v.transposed ? ((uint64_t)args.D * (uint64_t)v.ld + 192) : (seq + 192) * (uint64_t)v.ld) * (v.precision == PREC_FP32 ? 4u : 2u);
    if (bytes >= 0xFF000000ull) return false;
  }
  return true;
}

struct LaunchPlan {
  KernelArgs args;
  dim3 grid;
  const VariantInfo *variant;
  const Route *route;           // of `variant`, for this launch
  bool useFallback;
  uint32_t splits = 1;          // > 1: column-parallel forward through the caller's workspace
  float *wsO = nullptr, *wsML = nullptr;
  // transposed operands served through row-major copies in the caller's workspace
  struct Relayout { int slot; OperandView user; void *copy; uint32_t seq; uint32_t heads; bool output; };
  Relayout relayouts[MFA_BUFFER_SLOTS];
  int nRelayouts = 0;
  uint32_t heads = 1, batches = 1;
  // grouped-query backwardKeyValue (G = headsPerKeyValue > 1): the kernels write per-query-head fp32 slabs (wsKV: dV slabs, then dK
  // slabs) and attn_kv_group_sum stores their group sums through the caller's views kvOut (dV, dK)
  uint32_t groups = 1;
  float *wsKV = nullptr;
  OperandView kvOut[2];
  // a transposed backward launch without a workspace that the in-place kernels take (attn_bwd16_p4_tr.hip; AttentionKernel.swift:
  // 189-204: the reference reads transposed operands in place in every kernel) instead of the general kernel
  bool inPlaceBackward = false;
};

// ---- re-layout pass: element (r, d) of a [seq][D] matrix between a transposed view ([D][seq], leading dimension ld) and a
// compact row-major copy ([seq][D]); 64 x 64 tiles through LDS, 16-byte accesses on both sides.  HBM-bound: 2 x seq x D x size bytes.
}  // extern "C"
template <typename E>
static __global__ __launch_bounds__(256) void attn_relayout(const char *tptr, char *cptr, uint32_t seq, uint32_t D, int64_t tld,
                                                            int64_t theadStride, int64_t tbatchStride, uint32_t heads, int toTransposed) {
  // 64 x 64 tile, 16-byte global accesses on both sides (V elements each), element-wise through LDS in between
  constexpr int V = 16 / sizeof(E), T = 64, CH = T / V;      // chunks of V elements per tile row
  __shared__ E tile[T][T + 2];
  const uint32_t tilesD = (D + T - 1) / T;
  const uint32_t r0 = (blockIdx.x / tilesD) * T, d0 = (blockIdx.x % tilesD) * T;
  const uint32_t head = blockIdx.y, batch = blockIdx.z;
  E *tview = const_cast<E *>(reinterpret_cast<const E *>(tptr)) + (int64_t)head * theadStride + (int64_t)batch * tbatchStride;
  E *copy = reinterpret_cast<E *>(cptr) + ((int64_t)batch * heads + head) * (int64_t)seq * D;
  typedef E vec __attribute__((ext_vector_type(V)));
  // the 16-byte path needs whole chunks inside the matrix and 16-byte aligned rows on both sides
  const bool wide = (seq % V) == 0 && (D % V) == 0 && (tld % V) == 0 && ((reinterpret_cast<uintptr_t>(tview) | reinterpret_cast<uintptr_t>(copy)) & 15) == 0;
  // transposed view: rows = d, contiguous along the sequence; copy: rows = sequence position, contiguous along d
  for (int c = threadIdx.x; c < T * CH; c += 256) {          // load: tile[d][r] always
    const uint32_t a = c / CH, b = (c % CH) * V;              // row a of the SOURCE tile, elements b .. b+V-1
    if (!toTransposed) {                                      // source = transposed view: row a = d, elements = sequence
      const uint32_t d = d0 + a, r = r0 + b;
      if (d < D && wide && r + V <= seq) {
        const vec x = *reinterpret_cast<const vec *>(tview + (int64_t)d * tld + r);
#pragma unroll
        for (int k = 0; k < V; ++k) tile[a][b + k] = x[k];
      } else if (d < D) {
        for (int k = 0; k < V; ++k) if (r + k < seq) tile[a][b + k] = tview[(int64_t)d * tld + r + k];
      }
    } else {                                                  // source = row-major copy: row a = sequence, elements = d
      const uint32_t r = r0 + a, d = d0 + b;
      if (r < seq && wide && d + V <= D) {
        const vec x = *reinterpret_cast<const vec *>(copy + (int64_t)r * D + d);
#pragma unroll
        for (int k = 0; k < V; ++k) tile[b + k][a] = x[k];
      } else if (r < seq) {
        for (int k = 0; k < V; ++k) if (d + k < D) tile[b + k][a] = copy[(int64_t)r * D + d + k];
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < T * CH; c += 256) {          // store
    const uint32_t a = c / CH, b = (c % CH) * V;
    if (!toTransposed) {                                      // destination = copy: row a = sequence, elements = d
      const uint32_t r = r0 + a, d = d0 + b;
      if (r < seq && wide && d + V <= D) {
        vec x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = tile[b + k][a];
        *reinterpret_cast<vec *>(copy + (int64_t)r * D + d) = x;
      } else if (r < seq) {
        for (int k = 0; k < V; ++k) if (d + k < D) copy[(int64_t)r * D + d + k] = tile[b + k][a];
      }
    } else {                                                  // destination = transposed view: row a = d, elements = sequence
      const uint32_t d = d0 + a, r = r0 + b;
      if (d < D && wide && r + V <= seq) {
        vec x;
#pragma unroll
        for (int k = 0; k < V; ++k) x[k] = tile[a][b + k];
        *reinterpret_cast<vec *>(tview + (int64_t)d * tld + r) = x;
      } else if (d < D) {
        for (int k = 0; k < V; ++k) if (r + k < seq) tview[(int64_t)d * tld + r + k] = tile[a][b + k];
      }
    }
  }
}

extern "C" {

static hipError_t launch_relayout(const LaunchPlan &plan, const LaunchPlan::Relayout &r, hipStream_t stream) {
  const uint32_t D = plan.args.D;
  const dim3 grid(((r.seq + 63) / 64) * ((D + 63) / 64), r.heads, plan.batches);
  const char *t = static_cast<const char *>(r.user.ptr);
  char *c = static_cast<char *>(r.copy);
  const int toTransposed = r.output ? 1 : 0;
  if (r.user.precision == PREC_FP32)
    return launch_kernel(&attn_relayout<uint32_t>, grid, dim3(256), 0, stream, t, c, r.seq, D, r.user.ld, r.user.headStride, r.user.batchStride, r.heads, toTransposed);
  return launch_kernel(&attn_relayout<uint16_t>, grid, dim3(256), 0, stream, t, c, r.seq, D, r.user.ld, r.user.headStride, r.user.batchStride, r.heads, toTransposed);
}

static bool is_output_slot(int type, int slot) {
  switch (type) {
    case MFA_FORWARD: return slot == SLOT_O;
    case MFA_BACKWARD_QUERY: return slot == SLOT_dQ;
    default: return slot == SLOT_dK || slot == SLOT_dV;
  }
}

// grouped-query attention: G query heads per K / V head (mfa_launch_params.headsPerKeyValue; 0 and 1 = one K / V head per query head)
static uint32_t heads_per_kv(const mfa_launch_params *p) { return p->headsPerKeyValue > 1 ? p->headsPerKeyValue : 1; }
static bool kv_slot(int slot) { return slot == SLOT_K || slot == SLOT_V || slot == SLOT_dK || slot == SLOT_dV; }
// a grouped-query backwardKeyValue launch: dK / dV go through per-query-head slabs and attn_kv_group_sum
static bool grouped_dkv(const mfa_attention_kernel *kernel, uint32_t G) { return G > 1 && kernel->desc.type == MFA_BACKWARD_KEY_VALUE; }

// the K / V head of a query head: h / G as (umulhi(h, m) + h) >> l (kv_head, attn_common.h) with l = ceil(log2 G) and
// m = floor(2^32 (2^l - G) / G) + 1 -- i.e. floor(h M / 2^(32 + l)) with M = 2^32 + m = floor(2^(32 + l) / G) + 1, whose error
// h (MG - 2^(32 + l)) / (G 2^(32 + l)) < h / 2^(32 + l) stays below 1 / G for h < 2^16 (heads <= 65535): exact.  G = 1: (0, 0)
static void set_head_divisor(KernelArgs &a, uint32_t G) {
  a.kvHeadMul = a.kvHeadShift = 0;
  if (G <= 1) return;
  uint32_t l = 0;
  while ((1u << l) < G) ++l;
  a.kvHeadShift = l;
  a.kvHeadMul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - G)) / G + 1);
}

// The operands of a launch that go through row-major copies in the workspace: the transposed matrix operands of the kernel type.
// Grouped-query backwardKeyValue writes dK^T / dV^T in place (attn_kv_group_sum): no copy of them
static bool relayout_slot(const mfa_attention_kernel *kernel, int slot, uint32_t G) {
  if (!slot_used(kernel->desc.type, slot) || slot == SLOT_L || slot == SLOT_D) return false;
  if (grouped_dkv(kernel, G) && (slot == SLOT_dK || slot == SLOT_dV)) return false;
  return kernel->desc.transposeState[slot_operand(slot)] != 0;
}
// one such copy: its sequence length, its heads (K / V copies hold the Hq / G K / V heads, addressed through kv_head) and its bytes
// (256-byte aligned)
struct RelayoutCopy { uint32_t seq, heads; uint64_t bytes; };
static RelayoutCopy relayout_copy(const mfa_attention_kernel *kernel, int slot, uint32_t row, uint32_t column, uint32_t heads,
                                  uint32_t batches, uint32_t G) {
  const int op = slot_operand(slot);
  const uint32_t seq = row_operand(op) ? row : column;
  const uint32_t h = kv_slot(slot) ? heads / G : heads;
  const uint64_t esz = kernel->desc.memoryPrecisions[op] == MFA_FP32 ? 4 : 2;
  return {seq, h, ((uint64_t)h * batches * seq * kernel->desc.headDimension * esz + 255) & ~255ull};
}

// Column-parallel heuristic: split only when the row-parallel grid cannot fill the 256 CUs and the traversal is long enough to
// amortise the combine pass; keep >= 4 key tiles (256 keys) per piece.
// `target`: workgroups the variant wants in flight (512 = two per compute unit; 256 for the kernels that own a compute unit's whole
// register file and run one workgroup per compute unit -- a second round of half-length pieces would pay the per-block cost twice).
// Round 6 (tools/sweep_splits.py, profiles/r06_sweep_splits.txt): (1) the count is rounded DOWN to the target: 24 blocks x 11 pieces
// = 264 workgroups ran a second round of eight (N = 6144, one head: 33.8 us against 26.4 with 8 pieces); (2) more pieces shorten a
// piece's traversal by t_tile / s but every piece adds a slab to the combine pass (s x parallel x (D + 2) floats read back): the sum has
// its minimum at s^2 = K x traversal / parallel with K ~ 117 for every head dimension (a tile's time and a slab's bytes both grow
// with D), i.e. ~11 pieces for a square problem -- N = 4096 D = 64 one head forward: 21.0 us with 8 pieces, 23.5 with 16.
static uint32_t choose_splits(uint64_t blocks, uint32_t traversal, uint32_t parallel, uint32_t target = 512) {
  const uint32_t tiles = (traversal + 63) / 64;
  if (blocks >= 192 || tiles < 8) return 1;
  uint64_t s = target / blocks;
  // the cap ~ round(sqrt(117 t / p)): the largest b >= 1 with b (b - 1) p <= 117 t, i.e. b (b - 1) <= q -- the square root's estimate
  // is off by at most one either way
  const uint64_t q = 117ull * traversal / parallel;
  uint64_t best = (1 + (uint64_t)std::sqrt(4.0 * (double)q + 1.0)) / 2;
  while (best > 1 && best * (best - 1) > q) --best;
  while ((best + 1) * best <= q) ++best;
  if (s > best) s = best;
#ifdef MFA_DEV_VARIANTS
  if (const char *knob = std::getenv("MFA_SPLITS")) s = (uint64_t)std::atoi(knob);   // developer library: sweep of the piece count (tools/sweep_splits.py)
#endif
  if (s > tiles / 4) s = tiles / 4;
  if (s > 64) s = 64;
  // equal pieces of whole 256-key blocks when a count between s / 2 and s gives them (what the persistent forward kernels' split
  // streams serve: attn_fwd16_p4p.hip, attn_fwd16_p6.hip)
  for (uint64_t c = s; c >= 2 && 2 * c > s; --c)
    if (traversal % (256 * c) == 0) { s = c; break; }
  return s < 2 ? 1 : (uint32_t)s;
}

// column-parallel geometry of a launch on split route `r` (workspace query and launch alike): workgroups along the parallelization
// dimension and pieces of the traversal (1: no split)
struct SplitGeometry { uint32_t blocks, splits; };
static SplitGeometry split_geometry(const Route &r, int type, uint32_t row, uint32_t column, uint32_t heads, uint32_t batches) {
  const bool kv = type == MFA_BACKWARD_KEY_VALUE;
  const uint32_t par = kv ? column : row;   // (SquareAttentionTest.swift:355-367)
  const uint32_t blocks = (par + r.parallelization - 1) / r.parallelization;
  return {blocks, choose_splits((uint64_t)blocks * heads * batches, kv ? row : column, par, r.splitTarget ? r.splitTarget : 512)};
}

// bytes of workspace a launch cut into `s` pieces needs
static uint64_t split_workspace_bytes(int type, uint32_t s, uint32_t heads, uint32_t batches, uint32_t row, uint32_t column, uint32_t D) {
  const uint64_t hb = (uint64_t)heads * batches;
  if (type == MFA_FORWARD) return (uint64_t)s * hb * row * (D + 2) * sizeof(float);          // O slabs + (m, l)
  if (type == MFA_BACKWARD_QUERY) return (uint64_t)s * hb * row * D * sizeof(float);         // dQ slabs
  return 2ull * s * hb * column * D * sizeof(float);                                         // dV slabs, then dK slabs
}

// What a launch needs of the caller's workspace: the one answer behind mfa_attention_kernel_workspace_size and prepare_launch.
//   SLABS     grouped-query backwardKeyValue: the fp32 dV and dK slabs [batch][query head][column][D], then (256-byte aligned, at
//             relayoutOffset) the row-major copies of its transposed inputs; required, whatever the launch would otherwise do
//   RELAYOUT  row-major copies of the transposed operands (without them the launch runs the general kernel)
//   SPLIT     partial results of a traversal-parallel launch, for grids that cannot fill the GPU (without it the launch is not split)
struct WorkspaceNeed {
  enum Kind { NONE, SLABS, RELAYOUT, SPLIT } kind = NONE;
  uint64_t bytes = 0;
  uint64_t relayoutOffset = 0;
  const Route *splitRoute = nullptr;   // SPLIT: the variant's route of the pieces and their geometry
  SplitGeometry split = {0, 1};
};
static WorkspaceNeed workspace_need(const mfa_attention_kernel *kernel, uint32_t row, uint32_t column, uint32_t heads, uint32_t batches,
                                    uint32_t G, bool causal, bool hasLengths, bool hasMask) {
  WorkspaceNeed need;
  const int type = kernel->desc.type;
  const uint32_t D = kernel->desc.headDimension;
  if (grouped_dkv(kernel, G)) {
    need.kind = WorkspaceNeed::SLABS;
    need.bytes = 2ull * heads * batches * column * D * sizeof(float);
    need.relayoutOffset = (need.bytes + 255) & ~255ull;
  } else if (kernel->relayout) {
    need.kind = WorkspaceNeed::RELAYOUT;
  }
  if (kernel->relayout) {
    need.bytes = need.relayoutOffset;
    for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot)
      if (relayout_slot(kernel, slot, G)) need.bytes += relayout_copy(kernel, slot, row, column, heads, batches, G).bytes;
  }
  if (need.kind != WorkspaceNeed::NONE) return need;
  // (grouped-query backwardKeyValue is never split: its grid already spans the Hq query heads)
  const Route &split = kernel->variant.route(true, false, causal);
  if (!split || hasLengths || hasMask) return need;
  need.split = split_geometry(split, type, row, column, heads, batches);
  if (need.split.splits > 1) {
    need.kind = WorkspaceNeed::SPLIT;
    need.splitRoute = &split;
    need.bytes = split_workspace_bytes(type, need.split.splits, heads, batches, row, column, D);
  }
  return need;
}

// operand views and scalar arguments of a launch as the caller passed them
static mfa_status fill_args(const mfa_attention_kernel *kernel, void *const buffers[MFA_BUFFER_SLOTS], const mfa_launch_params *p,
                            KernelArgs *args) {
  const int type = kernel->desc.type;
  const uint32_t D = kernel->desc.headDimension;
  std::memset(args, 0, sizeof(*args));
  for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot) {
    if (!slot_used(type, slot)) continue;
    const int op = slot_operand(slot);
    if (!buffers[slot])
      return fail(MFA_ERR_INVALID_ARGUMENT, std::string("buffer for operand ") + mfa_operand_name(op) + " is null");
    OperandView &v = args->op[slot];
    v.ptr = buffers[slot];
    v.precision = kernel->desc.memoryPrecisions[op];
    const bool vector = (op == MFA_L || op == MFA_D);
    v.transposed = vector ? 0 : kernel->desc.transposeState[op];
    // sequence length of the operand (AttentionKernel.swift:157-187)
    const int64_t seq = (row_operand(op) || vector) ? p->row : p->column;
    int64_t ld = p->leadingDimension[slot];
    if (ld == 0) ld = v.transposed ? seq : (int64_t)D;  // AttentionKernel.swift:189-204
    if (!vector) {
      if (!v.transposed && ld < (int64_t)D) return fail(MFA_ERR_INVALID_ARGUMENT, "leading dimension smaller than head dimension");
      if (v.transposed && ld < seq) return fail(MFA_ERR_INVALID_ARGUMENT, "leading dimension smaller than sequence length");
    }
    v.ld = vector ? 1 : ld;
    v.headStride = p->headStride[slot];
    v.batchStride = p->batchStride[slot];
  }
  args->R = p->row;
  args->C = p->column;
  args->D = D;
  args->scale = 1.0f / std::sqrt((float)D);
  args->scale2 = 1.44269504089f / std::sqrt((float)D);
  args->causal = p->causal ? 1 : 0;
  args->rowLen = p->rowLengths;
  args->colLen = p->columnLengths;
  args->mask = p->blockMask;
  args->maskWords = p->blockMaskWords;
  args->maskHeadStride = p->blockMaskHeadStride;
  args->maskBatchStride = p->blockMaskBatchStride;
  if (p->blockMask && p->blockMaskWords * 32ull * MASK_BLOCK_COLUMNS < p->column)
    return fail(MFA_ERR_INVALID_ARGUMENT, "blockMaskWords does not cover `column`");
  if (p->causal && p->column < p->row)
    return fail(MFA_ERR_INVALID_ARGUMENT, "causal masking requires column >= row");
  return MFA_OK;
}

// grouped-query backwardKeyValue: dK / dV of every query head to fp32 slabs of the workspace; attn_kv_group_sum adds each group's
// slabs into the caller's views
static mfa_status take_group_slabs(const mfa_launch_params *p, const WorkspaceNeed &need, LaunchPlan *plan) {
  KernelArgs *args = &plan->args;
  const uint32_t D = args->D, heads = plan->heads;
  if (!p->workspace || p->workspaceBytes < need.bytes || (reinterpret_cast<uintptr_t>(p->workspace) & 255) != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "backwardKeyValue with headsPerKeyValue " + std::to_string(plan->groups) + " needs a 256-byte aligned workspace of " +
                                              std::to_string(need.bytes) + " bytes (mfa_attention_kernel_workspace_size) for its per-query-head dK / dV slabs");
  if ((uint64_t)p->column * D > 0xFFFFFFFFull - 255)
    return fail(MFA_ERR_INVALID_ARGUMENT, "backwardKeyValue with headsPerKeyValue > 1: column x head dimension must stay below 2^32");
  const uint64_t half = (uint64_t)heads * plan->batches * p->column * D;   // floats per slab set
  plan->wsKV = static_cast<float *>(p->workspace);
  plan->kvOut[0] = args->op[SLOT_dV];
  plan->kvOut[1] = args->op[SLOT_dK];
  for (int i = 0; i < 2; ++i) {
    OperandView &v = args->op[i ? SLOT_dK : SLOT_dV];
    v.ptr = plan->wsKV + i * half;
    v.precision = PREC_FP32; v.transposed = 0; v.ld = D;
    v.headStride = (int64_t)p->column * D; v.batchStride = (int64_t)heads * p->column * D;
  }
  return MFA_OK;
}

// Transposed operands of a kernel that runs on row-major copies: the views move onto copies in the workspace.  false: there is no
// (or too small / misaligned a) workspace -- the general kernel reads the transposed operands in place.
// Per-batch lengths: the matrix-core kernels never write the padding rows of an output, so the write-back of a row-major output
// copy (uninitialised workspace) would overwrite the caller's padding region -- such launches take the general kernel too
static bool take_relayout_copies(const mfa_attention_kernel *kernel, const mfa_launch_params *p, const WorkspaceNeed &need, LaunchPlan *plan) {
  KernelArgs *args = &plan->args;
  const bool lengths = args->rowLen || args->colLen;
  if (lengths || !p->workspace || p->workspaceBytes < need.bytes || (reinterpret_cast<uintptr_t>(p->workspace) & 255) != 0) return false;
  char *cursor = static_cast<char *>(p->workspace) + need.relayoutOffset;
  // (grouped-query backwardKeyValue: dK / dV are the slabs by now, row-major)
  for (int slot = 0; slot < MFA_BUFFER_SLOTS; ++slot) {
    if (!relayout_slot(kernel, slot, plan->groups)) continue;
    const RelayoutCopy c = relayout_copy(kernel, slot, p->row, p->column, plan->heads, plan->batches, plan->groups);
    OperandView &v = args->op[slot];
    LaunchPlan::Relayout &r = plan->relayouts[plan->nRelayouts++];
    r.slot = slot; r.user = v; r.copy = cursor; r.seq = c.seq; r.heads = c.heads; r.output = is_output_slot(kernel->desc.type, slot);
    cursor += c.bytes;
    v.ptr = r.copy; v.transposed = 0; v.ld = args->D;
    v.headStride = (int64_t)c.seq * args->D; v.batchStride = (int64_t)c.heads * c.seq * args->D;
  }
  return true;
}

// Which code object serves the launch: the selected variant, the general kernel (plan->useFallback) or, for a transposed backward
// launch without its workspace, the in-place kernels (plan->inPlaceBackward)
static mfa_status choose_code_object(const mfa_attention_kernel *kernel, const mfa_launch_params *p, const WorkspaceNeed &need, bool relayoutMissing,
                                     LaunchPlan *plan) {
  KernelArgs *args = &plan->args;
  const int type = kernel->desc.type;
  const bool otherReasons = !meets_fast_requirements(kernel, *args) || (args->causal && !kernel->variant.causal) ||
                            (args->mask && !kernel->variant.sparse) ||
                            // attn_dkv16_rs lists at most 4096 active 256-row blocks in LDS
                            (args->mask && type == MFA_BACKWARD_KEY_VALUE && p->row > 4096u * 256u);
  plan->useFallback = kernel->hasFallback && (relayoutMissing || otherReasons);
  // a transposed backward launch whose ONLY reason to leave the matrix-core kernel is the missing workspace (every operand meets the
  // alignment and 32-bit slice-size requirements of the buffer descriptors, which the in-place kernels address every operand
  // through) goes to the in-place kernels when they take it
  if (kernel->hasFallback && relayoutMissing && !otherReasons && type != MFA_FORWARD) {
    const Launch probe{*args, dim3(1, plan->heads, plan->batches), 1, nullptr, nullptr, nullptr, false, hipSuccess};
    plan->inPlaceBackward = bwd16_p4_tr_launch(type, kernel->desc.registerPrecisions[MFA_P] > MFA_FP32, probe) != nullptr;
  }
#ifdef MFA_DEV_VARIANTS
  const char *knob = std::getenv("MFA_BWD16_TR");   // developer library: MFA_BWD16_TR=0 -- never (A/B runs against the general kernel)
  if (knob && std::strcmp(knob, "0") == 0) plan->inPlaceBackward = false;
#endif
  // strictBlockDimensions: a backward launch on 16-bit transposed operands that has no workspace for the re-layout path and is not
  // one the in-place kernels take would run the general fp32 kernel -- 20-50 x slower than the code object the descriptor selected
  // (the reference reads transposed operands in place at every head dimension, AttentionKernel.swift:189-204).  A strict caller
  // gets an error that names the remedy instead of the silent fallback
  if (kernel->desc.strictBlockDimensions && kernel->hasFallback && relayoutMissing && type != MFA_FORWARD && !plan->inPlaceBackward) {
    return fail(MFA_ERR_UNSUPPORTED,
                std::string("strictBlockDimensions: this launch of ") + kernel->variant.name + " on transposed operands has no (or too small / "
                "misaligned) workspace and would run the general kernel " + kernel->fallback.name + "; pass a 256-byte aligned workspace of " +
                std::to_string(need.bytes) + " bytes (mfa_attention_kernel_workspace_size) for the re-layout path" +
                ((args->rowLen || args->colLen) ? " -- not available with per-batch lengths: store the operands row-major" : ""));
  }
  if (plan->useFallback && plan->nRelayouts) {   // (alignment, mask limits ...): the general kernel takes the user's views
    for (int i = 0; i < plan->nRelayouts; ++i) args->op[plan->relayouts[i].slot] = plan->relayouts[i].user;
    plan->nRelayouts = 0;
  }
  plan->variant = plan->useFallback ? &kernel->fallback : &kernel->variant;
  plan->route = &plan->variant->route(false, args->mask != nullptr, args->causal != 0);
  return MFA_OK;
}

// The grid of the plan's route; a launch that workspace_need would split is cut into pieces when the caller's workspace takes their
// partial results: forward cuts the key range (partial (O, m, l), online-softmax merge), backwardQuery the key range and
// backwardKeyValue the row range (partial dQ / dK, dV in fp32 slabs, summed by attn_bwd_combine)
static mfa_status plan_grid(const mfa_attention_kernel *kernel, const mfa_launch_params *p, const WorkspaceNeed &need, LaunchPlan *plan) {
  const uint32_t heads = plan->heads, batches = plan->batches, D = plan->args.D;
  // parallelization dimension: rows for forward / backwardQuery, columns for backwardKeyValue
  // (SquareAttentionTest.swift:355-367)
  const uint32_t par = (kernel->desc.type == MFA_BACKWARD_KEY_VALUE) ? p->column : p->row;
  const uint32_t blocks = (par + plan->route->parallelization - 1) / plan->route->parallelization;
  if ((uint64_t)blocks * heads * batches > 0x7FFFFFFFull) return fail(MFA_ERR_INVALID_ARGUMENT, "grid too large");
  plan->grid = dim3(blocks, heads, batches);
  plan->splits = 1;
  if (plan->useFallback || need.kind != WorkspaceNeed::SPLIT) return MFA_OK;
  const uint32_t s = need.split.splits;
  if (p->workspace && p->workspaceBytes >= need.bytes && (reinterpret_cast<uintptr_t>(p->workspace) & 15) == 0 && (D % 4) == 0 &&
      (uint64_t)need.split.blocks * heads * batches * s <= 0x7FFFFFFFull) {
    plan->route = need.splitRoute;
    plan->grid = dim3(need.split.blocks, heads, batches);
    plan->splits = s;
    plan->wsO = static_cast<float *>(p->workspace);
    plan->wsML = plan->wsO + (uint64_t)s * heads * batches * p->row * D;   // forward only
  }
  return MFA_OK;
}

static mfa_status prepare_launch(const mfa_attention_kernel *kernel, void *const buffers[MFA_BUFFER_SLOTS],
                                 const mfa_launch_params *p, LaunchPlan *plan) {
  if (!kernel || !buffers || !p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  if (p->row == 0 || p->column == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "row and column must be non-zero");
  mfa_status st = fill_args(kernel, buffers, p, &plan->args);
  if (st != MFA_OK) return st;
  const uint32_t heads = p->heads ? p->heads : 1, batches = p->batches ? p->batches : 1;
  if (heads > 65535 || batches > 65535) return fail(MFA_ERR_INVALID_ARGUMENT, "heads and batches must be <= 65535");
  plan->heads = heads;
  plan->batches = batches;
  plan->nRelayouts = 0;
  const uint32_t G = heads_per_kv(p);
  if (heads % G != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "heads (" + std::to_string(heads) + ") is not a multiple of headsPerKeyValue (" + std::to_string(G) + ")");
  plan->groups = G;
  set_head_divisor(plan->args, G);
  const WorkspaceNeed need = workspace_need(kernel, p->row, p->column, heads, batches, G, p->causal != 0,
                                            p->rowLengths || p->columnLengths, p->blockMask != nullptr);
  if (need.kind == WorkspaceNeed::SLABS) {
    st = take_group_slabs(p, need, plan);
    if (st != MFA_OK) return st;
  }
  const bool relayoutMissing = kernel->relayout && !take_relayout_copies(kernel, p, need, plan);
  st = choose_code_object(kernel, p, need, relayoutMissing, plan);
  if (st != MFA_OK) return st;
  return plan_grid(kernel, p, need, plan);
}

// The one route of a prepared launch, for mfa_attention_kernel_launch / _time (run) and _launch_form (not run; `form` receives the
// text): the in-place backward kernels, or the re-layout passes around the plan's route of its variant (split + combine, block-sparse,
// causal or dense).  Each entry point decides which code object serves the launch and names it.  Returns the first failed HIP call
// of a run.
static hipError_t run_plan(const mfa_attention_kernel *kernel, const LaunchPlan &plan, hipStream_t stream, bool run, std::string *form = nullptr) {
  const Launch l{plan.args, plan.grid, plan.splits, plan.wsO, plan.wsML, stream, run, hipSuccess};
  // grouped-query backwardKeyValue: the group sums of the per-query-head slabs into the caller's dK / dV
  auto group_sum = [&]() {
    if (plan.groups <= 1 || kernel->desc.type != MFA_BACKWARD_KEY_VALUE) return;
    const uint64_t half = (uint64_t)plan.heads * plan.batches * plan.args.C * plan.args.D;
    if (run && l.err == hipSuccess)
      l.err = launch_kv_group_sum(plan.wsKV, plan.wsKV + half, plan.kvOut[0], plan.kvOut[1], plan.groups, plan.heads / plan.groups,
                                  plan.batches, plan.args.C, plan.args.D, plan.args.colLen, stream);
    if (form) *form += " + attn_kv_group_sum x" + std::to_string(plan.groups);
  };
  if (plan.inPlaceBackward) {
    const char *chosen = bwd16_p4_tr_launch(kernel->desc.type, kernel->desc.registerPrecisions[MFA_P] > MFA_FP32, l);
    if (form) *form = chosen;
    group_sum();
    return l.err;
  }
  for (int i = 0; i < plan.nRelayouts && run && l.err == hipSuccess; ++i)
    if (!plan.relayouts[i].output) l.err = launch_relayout(plan, plan.relayouts[i], stream);
  const VariantInfo &v = *plan.variant;
  const Route &r = *plan.route;
  const char *chosen = r.launch(l);
  for (int i = 0; i < plan.nRelayouts && run && l.err == hipSuccess; ++i)
    if (plan.relayouts[i].output) l.err = launch_relayout(plan, plan.relayouts[i], stream);
  if (form) {
    std::string &text = *form;
    text = plan.nRelayouts ? "attn_relayout x" + std::to_string(plan.nRelayouts) + " + " : "";
    if (plan.useFallback) {
      text += std::string(chosen ? chosen : v.name) + " (general kernel: the launch does not meet the requirements of " + kernel->variant.name + ")";
    } else if (plan.splits > 1) {
      text += std::string(v.name) + " column-parallel x" + std::to_string(plan.splits) + " + combine";
      if (chosen) text += std::string(" (") + chosen + ")";
      else if (std::strcmp(r.owner, v.name)) text += std::string(" (pieces by the sibling kernel ") + r.owner + ")";
    } else {
      text += chosen ? chosen : v.name;
      // (a mask taken by the dense code object itself, attn_paged.h, is not a block-sparse code object)
      if (&r == &v.sparse && r.launch != v.dense.launch)
        text += std::strcmp(r.owner, v.name) ? std::string(" (block-sparse sibling ") + r.owner + ")" : std::string(" (block-sparse code object)");
    }
  }
  group_sum();
  return l.err;
}

static const char *plan_name(const LaunchPlan &plan) { return plan.inPlaceBackward ? "attn_bwd16_p4_tr" : plan.variant->name; }

mfa_status mfa_attention_kernel_launch(const mfa_attention_kernel *kernel, void *const buffers[MFA_BUFFER_SLOTS],
                                       const mfa_launch_params *params, void *stream) {
  LaunchPlan plan;
  mfa_status st = prepare_launch(kernel, buffers, params, &plan);
  if (st != MFA_OK) return st;
  hipError_t err = run_plan(kernel, plan, (hipStream_t)stream, true);
  if (err == hipSuccess) err = hipGetLastError();
#ifdef MFA_DEV_VARIANTS
  const char *knob = std::getenv("MFA_BWD16_TR");
  if (plan.inPlaceBackward && knob && std::strcmp(knob, "verbose") == 0)
    std::fprintf(stderr, "mfa: %s on transposed operands in place\n", kernel->desc.type == MFA_BACKWARD_QUERY ? "attn_dq16_p4_tr" : "attn_dkv16_p4_tr");
#endif
  if (err != hipSuccess) return hip_fail(err, plan_name(plan));
  return MFA_OK;
}

mfa_status mfa_attention_kernel_launch_form(const mfa_attention_kernel *kernel, void *const buffers[MFA_BUFFER_SLOTS],
                                            const mfa_launch_params *params, char *out, size_t capacity) {
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  LaunchPlan plan;
  mfa_status st = prepare_launch(kernel, buffers, params, &plan);
  if (st != MFA_OK) return st;
  std::string text;
  (void)run_plan(kernel, plan, nullptr, false, &text);   // (nothing is started: no HIP call)
  copy_text(out, capacity, text.c_str());
  return MFA_OK;
}

mfa_status mfa_attention_kernel_workspace_size(const mfa_attention_kernel *kernel, const mfa_launch_params *params,
                                               uint64_t *bytes) {
  if (!kernel || !params || !bytes) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = 0;
  if (params->row == 0 || params->column == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "row and column must be non-zero");
  const uint32_t G = heads_per_kv(params), H = params->heads ? params->heads : 1, B = params->batches ? params->batches : 1;
  if (H % G != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "heads (" + std::to_string(H) + ") is not a multiple of headsPerKeyValue (" + std::to_string(G) + ")");
  *bytes = workspace_need(kernel, params->row, params->column, H, B, G, params->causal != 0,
                          params->rowLengths || params->columnLengths, params->blockMask != nullptr).bytes;
  return MFA_OK;
}

mfa_status mfa_attention_kernel_time(const mfa_attention_kernel *kernel, void *const buffers[MFA_BUFFER_SLOTS],
                                     const mfa_launch_params *params, void *stream, int warmup, int iterations,
                                     float *milliseconds) {
  if (!milliseconds || iterations <= 0 || warmup < 0) return fail(MFA_ERR_INVALID_ARGUMENT, "bad timing arguments");
  LaunchPlan plan;
  mfa_status st = prepare_launch(kernel, buffers, params, &plan);
  if (st != MFA_OK) return st;
  // (a code object's first launch on a device raises its LDS limit, a host-side call: with warmup = 0 the first timed launch pays it)
  return time_launches((hipStream_t)stream, warmup, iterations, milliseconds, plan_name(plan),
                       [&](hipStream_t s) { return run_plan(kernel, plan, s, true); });
}

mfa_status mfa_device_count(int *count) {
  if (!count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  hipError_t err = hipGetDeviceCount(count);
  if (err != hipSuccess) { *count = 0; return hip_fail(err, "hipGetDeviceCount"); }
  return MFA_OK;
}

mfa_status mfa_device_name(int device, char *out, size_t capacity) {
  if (!out || capacity == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  hipDeviceProp_t prop;
  hipError_t err = hipGetDeviceProperties(&prop, device);
  if (err != hipSuccess) return hip_fail(err, "hipGetDeviceProperties");
  copy_text(out, capacity, prop.gcnArchName);
  return MFA_OK;
}

} // extern "C"
