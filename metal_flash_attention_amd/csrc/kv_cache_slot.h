// kv_cache_slot.h -- where key `pos` of sequence `batch` lies in a KV cache that a launch WRITES (kv_cache_append.hip,
// kv_cache_compact.hip), and the one statement of the rows such a launch drops (include/mfa_kvcache.h): a negative position, a
// position at or past `column` of a contiguous cache, a page index at or past the block table's stride, a negative table entry.
// Device code, inlined.
#pragma once
#include <cstdint>

namespace mfa {

// false: the row is dropped.  Otherwise the row of head 0 starts at  *outer x (paged ? pageStride : batchStride) + *in x leadingDimension
// elements: *outer is the page (paged) or the sequence, *in the key inside it.
__device__ __forceinline__ bool kv_cache_slot(const int32_t *table, int64_t tableStride, uint32_t paged, uint32_t pageShift, uint32_t column,
                                              uint32_t batch, int64_t pos, int64_t *outer, int64_t *in) {
  if (pos < 0) return false;
  if (paged) {
    const int64_t pageIndex = pos >> pageShift;
    if (pageIndex >= tableStride) return false;
    const int64_t page = (int64_t)table[(int64_t)batch * tableStride + pageIndex];
    if (page < 0) return false;
    *outer = page;
    *in = pos & (((int64_t)1 << pageShift) - 1);
  } else {
    if (pos >= (int64_t)column) return false;
    *outer = (int64_t)batch;
    *in = pos;
  }
  return true;
}

} // namespace mfa
