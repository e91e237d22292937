// kv_cache_compact.hip -- moves the K and V rows of the accepted speculation-tree path to the front of the tree's slots, in place
// (include/mfa_compact.h).  One workgroup per (sequence, K or V, K/V head): it owns one slab of at most 64 rows, which no other
// workgroup touches.  Every lane LOADS its 16-byte pieces of the accepted rows into registers (64 rows x 512 B over 256 lanes: at most
// 8 pieces a lane), waits for them, passes the workgroup barrier and only then STORES them: every source is read before any destination
// is written, so paths that rotate, reverse or repeat nodes move what stood there before the launch.  Only the bytes of a row matter to
// a move: one kernel per byte count serves bf16, f16 and e4m3 caches.  The address of a key and the rows that are dropped are the
// append launch's (kv_cache_slot.h), the host's paging, stride and buffer checks too (cache_launch.h).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <string>

#include "../../include/mfa_compact.h"
#include "attn_common.h"
#include "cache_launch.h"
#include "kv_cache_slot.h"
#include "launchers.h"
#include "mfa_internal.h"

using namespace mfa;

namespace {

struct CompactArgs {
  char *cache[2];                 // kCache, vCache
  const uint32_t *lengths, *qlens;
  const int32_t *table;
  int64_t tableStride;
  const int32_t *accepted;
  int64_t acceptedStride;
  const uint32_t *counts;
  uint32_t *newLengths;
  int64_t ldc[2], hsc[2], osc[2]; // elements; osc: the batch stride, or the page stride of a paged cache
  uint32_t R, H, column, maxAccepted;
  uint32_t paged, pageShift, elementShift;   // an element is 1 << elementShift bytes
};

template <int BYTES>
__device__ __forceinline__ void kv_compact_body(const CompactArgs &a) {
  constexpr uint32_t CPR = BYTES / 16;                           // 16-byte pieces per row
  constexpr int PIECES = (int)(MFA_TREE_MAX_NODES * CPR / 256);  // ... per lane: 1, 2, 4, 8
  const uint32_t head = blockIdx.x % a.H, o = (blockIdx.x / a.H) & 1u, batch = blockIdx.x / (2u * a.H);
  const uint32_t length = a.lengths[batch];
  const uint32_t n = a.paged || length < a.column ? length : a.column;
  const uint32_t given = a.qlens ? a.qlens[batch] : a.R, qn = given < a.R ? given : a.R;
  const uint32_t P = n > qn ? n - qn : 0u, live = qn < n ? qn : n;
  uint32_t count = a.counts[batch];
  count = count < a.maxAccepted ? count : a.maxAccepted;
  count = count < live ? count : live;
  if (a.newLengths && o == 0 && head == 0 && threadIdx.x == 0) a.newLengths[batch] = P + count;
  char *const cache = o ? a.cache[1] : a.cache[0];
  const int64_t ld = o ? a.ldc[1] : a.ldc[0], outerStride = o ? a.osc[1] : a.osc[0];
  const int64_t headAt = (int64_t)head * (o ? a.hsc[1] : a.hsc[0]);

  // where this lane's pieces come from and go to: the dependent loads (the path, the block table) of all pieces first, ...
  int64_t from[PIECES], at[PIECES];
  uint32_t moved = 0;   // bit t: piece t of this lane is moved
#pragma unroll
  for (int t = 0; t < PIECES; ++t) {
    const uint32_t idx = threadIdx.x + 256u * t, i = idx / CPR, c = idx % CPR;
    from[t] = at[t] = 0;
    if (i < count) {
      const int32_t j = a.accepted[(int64_t)batch * a.acceptedStride + i];
      int64_t so, si, dso, dsi;
      if (j >= 0 && (uint32_t)j < live && (uint32_t)j != i &&   // (j == i: the row is in place already)
          kv_cache_slot(a.table, a.tableStride, a.paged, a.pageShift, a.column, batch, (int64_t)P + j, &so, &si) &&
          kv_cache_slot(a.table, a.tableStride, a.paged, a.pageShift, a.column, batch, (int64_t)P + i, &dso, &dsi)) {
        from[t] = ((so * outerStride + si * ld + headAt) << a.elementShift) + 16 * c;
        at[t] = ((dso * outerStride + dsi * ld + headAt) << a.elementShift) + 16 * c;
        moved |= 1u << t;
      }
    }
  }
  // ... then the rows themselves, unconditionally so that all are in flight together: a piece that is not moved reads the first 16
  // bytes of the cache (from = 0, always inside the buffer) and is never stored
  u32x4 x[PIECES];
#pragma unroll
  for (int t = 0; t < PIECES; ++t) x[t] = *reinterpret_cast<const u32x4 *>(cache + from[t]);
  // every load of every lane has landed in its registers before any lane of the workgroup stores
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int t = 0; t < PIECES; ++t)
    if (moved & (1u << t)) *reinterpret_cast<u32x4 *>(cache + at[t]) = x[t];
}

} // namespace

#define MFA_KV_COMPACT_KERNEL(BYTES)                                                                                                  \
  extern "C" __global__ __launch_bounds__(256) void kv_cache_compact_b##BYTES(const CompactArgs a) { kv_compact_body<BYTES>(a); }
MFA_KV_COMPACT_KERNEL(64)
MFA_KV_COMPACT_KERNEL(128)
MFA_KV_COMPACT_KERNEL(256)
MFA_KV_COMPACT_KERNEL(512)

namespace {

typedef void (*CompactKernel)(const CompactArgs);
struct CompactEntry {
  uint32_t bytes;
  CompactKernel launch;
  const char *name;
};
#define MFA_KV_COMPACT_ENTRY(BYTES) {BYTES, kv_cache_compact_b##BYTES, "kv_cache_compact_b" #BYTES}
const CompactEntry kKernels[] = {MFA_KV_COMPACT_ENTRY(64), MFA_KV_COMPACT_ENTRY(128), MFA_KV_COMPACT_ENTRY(256), MFA_KV_COMPACT_ENTRY(512)};

mfa_status prepare(const mfa_kv_compact_params *p, CompactArgs *a, const CompactEntry **entry) {
  if (!p) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  bool fp8;
  mfa_status st = check_cache_precision(p->cachePrecision, &fp8);
  if (st != MFA_OK) return st;
  if (!fp8 && p->cachePrecision != MFA_BF16 && p->cachePrecision != MFA_FP16)
    return fail(MFA_ERR_INVALID_ARGUMENT, "cachePrecision must be the cache's 16-bit type (MFA_FP16 or MFA_BF16) or MFA_KV_E4M3");
  if (p->headDimension != 64 && p->headDimension != 128 && p->headDimension != 256)
    return fail(MFA_ERR_UNSUPPORTED, "the KV cache compaction is compiled for head dimensions 64, 128 and 256, not " + std::to_string(p->headDimension));
  if (p->rows == 0 || p->heads == 0 || p->batches == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "rows, heads and batches must be non-zero");
  if (2ull * p->heads * p->batches > 0x7FFFFFFFull)
    return fail(MFA_ERR_INVALID_ARGUMENT, "2 x heads x batches must fit a grid of 2^31 - 1 workgroups");
  if (p->rows > MFA_TREE_MAX_NODES || p->maxAccepted > MFA_TREE_MAX_NODES)
    return fail(MFA_ERR_UNSUPPORTED, "a speculation tree holds at most " + std::to_string(MFA_TREE_MAX_NODES) + " nodes: rows = " +
                                         std::to_string(p->rows) + ", maxAccepted = " + std::to_string(p->maxAccepted));
  if (p->maxAccepted == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "maxAccepted must be non-zero (the most rows a sequence moves, 1 to 64)");
  if (p->acceptedStride < (int64_t)p->maxAccepted)
    return fail(MFA_ERR_INVALID_ARGUMENT, "acceptedStride must be at least maxAccepted elements: a sequence's path is one row of `accepted`");
  if (!p->cacheLengths) return fail(MFA_ERR_INVALID_ARGUMENT, "cacheLengths is required (device array of `batches` uint32)");
  if (!p->accepted)
    return fail(MFA_ERR_INVALID_ARGUMENT, "accepted is required (device array of int32, [batches][acceptedStride]: the path's node indices, root first)");
  if (!p->acceptedCounts) return fail(MFA_ERR_INVALID_ARGUMENT, "acceptedCounts is required (device array of `batches` uint32)");
  if ((uintptr_t)p->accepted % 4) return fail(MFA_ERR_INVALID_ARGUMENT, "accepted must be 4-byte aligned");
  if (p->newLengths) {
    const uintptr_t lo = (uintptr_t)p->newLengths, other = (uintptr_t)p->cacheLengths, span = 4ull * p->batches;
    if (lo < other + span && other < lo + span)
      return fail(MFA_ERR_INVALID_ARGUMENT, "newLengths must not overlap cacheLengths: workgroups still read a sequence's old length "
                                            "after another has written its new one");
    if (lo % 4) return fail(MFA_ERR_INVALID_ARGUMENT, "newLengths must be 4-byte aligned");
  }
  uint32_t pageShift = 0;
  st = check_written_cache(p->pageSize, p->blockTable, p->blockTableStride, p->column, &pageShift);
  if (st != MFA_OK) return st;
  static const char *names[2] = {"kCache", "vCache"};
  for (int o = 0; o < 2; ++o) {
    st = check_written_cache_strides(names[o], p->headDimension, p->leadingDimension[o], p->headStride[o],
                                     p->pageSize ? p->pageStride[o] : p->batchStride[o], fp8);
    if (st != MFA_OK) return st;
  }
  std::memset(a, 0, sizeof(*a));
  a->lengths = p->cacheLengths; a->qlens = p->queryLengths;
  a->table = p->blockTable; a->tableStride = p->blockTableStride;
  a->accepted = p->accepted; a->acceptedStride = p->acceptedStride; a->counts = p->acceptedCounts; a->newLengths = p->newLengths;
  for (int o = 0; o < 2; ++o) {
    a->ldc[o] = p->leadingDimension[o]; a->hsc[o] = p->headStride[o];
    a->osc[o] = p->pageSize ? p->pageStride[o] : p->batchStride[o];
  }
  a->R = p->rows; a->H = p->heads; a->column = p->column; a->maxAccepted = p->maxAccepted;
  a->paged = p->pageSize != 0; a->pageShift = pageShift; a->elementShift = fp8 ? 0 : 1;
  const uint32_t bytes = (uint32_t)p->headDimension << a->elementShift;
  for (const CompactEntry &e : kKernels)
    if (e.bytes == bytes) *entry = &e;
  return MFA_OK;
}

} // namespace

extern "C" {

void mfa_kv_compact_params_init(mfa_kv_compact_params *params) {
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->cachePrecision = MFA_BF16;
}

size_t mfa_kv_compact_params_size(void) { return sizeof(mfa_kv_compact_params); }

mfa_status mfa_kv_compact_params_offsets(uint32_t *offsets, uint32_t capacity, uint32_t *count) {
  if (!offsets || !count) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
#define MFA_AT(FIELD) (uint32_t)offsetof(mfa_kv_compact_params, FIELD)
  static const uint32_t table[] = {MFA_AT(rows), MFA_AT(heads), MFA_AT(batches), MFA_AT(column), MFA_AT(headDimension), MFA_AT(cachePrecision),
                                   MFA_AT(reserved), MFA_AT(pageSize), MFA_AT(cacheLengths), MFA_AT(queryLengths), MFA_AT(blockTable),
                                   MFA_AT(blockTableStride), MFA_AT(accepted), MFA_AT(acceptedStride), MFA_AT(acceptedCounts), MFA_AT(maxAccepted),
                                   MFA_AT(reserved2), MFA_AT(newLengths), MFA_AT(leadingDimension), MFA_AT(headStride), MFA_AT(batchStride),
                                   MFA_AT(pageStride)};
#undef MFA_AT
  const uint32_t fields = (uint32_t)(sizeof(table) / sizeof(table[0]));
  *count = fields;
  for (uint32_t i = 0; i < fields && i < capacity; ++i) offsets[i] = table[i];
  return MFA_OK;
}

mfa_status mfa_kv_cache_compact_launch(void *kCache, void *vCache, const mfa_kv_compact_params *params, void *stream) {
  CompactArgs a;
  const CompactEntry *entry = nullptr;
  mfa_status st = prepare(params, &a, &entry);
  if (st == MFA_OK) st = check_buffers({kCache, vCache}, "kCache and vCache");
  if (st != MFA_OK) return st;
  a.cache[0] = (char *)kCache; a.cache[1] = (char *)vCache;
  hipError_t err = launch_kernel(entry->launch, dim3(2u * params->heads * params->batches), dim3(256), 0, (hipStream_t)stream, a);
  if (err == hipSuccess) err = hipGetLastError();
  if (err != hipSuccess) return hip_fail(err, entry->name);
  return MFA_OK;
}

} // extern "C"
