// cache_launch.cpp -- the host checks the launches over a KV cache share (cache_launch.h).
#include "cache_launch.h"

#include <cstring>
#include <cmath>
#include <string>

#include "../../include/mfa_kvcache.h"

namespace mfa {

mfa_status hip_fail(hipError_t err, const char *what) {
  return fail(MFA_ERR_HIP, std::string(what) + ": " + hipGetErrorName(err) + " (" + hipGetErrorString(err) + ")");
}

void copy_text(char *out, size_t capacity, const char *text) {
  std::strncpy(out, text, capacity - 1);
  out[capacity - 1] = '\0';
}

mfa_status check_paging(uint32_t pageSize, const void *blockTable, int64_t blockTableStride, uint32_t column, uint32_t *pageShift) {
  *pageShift = 0;
  if (!pageSize) return MFA_OK;
  if (pageSize < 16 || pageSize > 1024 || (pageSize & (pageSize - 1)))
    return fail(MFA_ERR_INVALID_ARGUMENT, "pageSize must be a power of two from 16 to 1024 (or 0: contiguous), not " + std::to_string(pageSize));
  if (!blockTable) return fail(MFA_ERR_INVALID_ARGUMENT, "a paged launch (pageSize != 0) needs blockTable");
  if (column) {
    const int64_t pagesPerSequence = ((int64_t)column + pageSize - 1) / pageSize;
    if (blockTableStride < pagesPerSequence)
      return fail(MFA_ERR_INVALID_ARGUMENT, "blockTableStride must hold the " + std::to_string(pagesPerSequence) + " pages of `column` keys");
  } else if (blockTableStride <= 0) {
    return fail(MFA_ERR_INVALID_ARGUMENT, "blockTableStride must be positive: the pages a sequence may name");
  }
  while ((1u << *pageShift) < pageSize) ++*pageShift;
  return MFA_OK;
}

mfa_status check_written_cache(uint32_t pageSize, const void *blockTable, int64_t blockTableStride, uint32_t column, uint32_t *pageShift) {
  const mfa_status st = check_paging(pageSize, blockTable, blockTableStride, 0, pageShift);   // (0: the kernel drops a row past the stride)
  if (st != MFA_OK) return st;
  if (!pageSize && column == 0) return fail(MFA_ERR_INVALID_ARGUMENT, "column (the capacity of a contiguous cache) must be non-zero");
  return MFA_OK;
}

const char *const kWrittenCacheStridesWhy = "(16-byte rows of 16-bit operands; an e4m3 cache: multiples of 16 elements)";

mfa_status check_written_cache_strides(const char *name, uint32_t headDimension, int64_t leadingDimension, int64_t headStride, int64_t outer, bool fp8) {
  return check_operand_strides(name, headDimension, leadingDimension, headStride, outer, fp8 ? 16 : 8, kWrittenCacheStridesWhy);
}

mfa_status check_stride_multiples(const char *name, int64_t leadingDimension, int64_t headStride, int64_t outer, int64_t need, const char *why) {
  if (leadingDimension % need || headStride % need || outer % need)
    return fail(MFA_ERR_INVALID_ARGUMENT, std::string("strides of ") + name + " must be multiples of " + std::to_string(need) + " elements " + why);
  return MFA_OK;
}

mfa_status check_operand_strides(const char *name, uint32_t headDimension, int64_t leadingDimension, int64_t headStride, int64_t outer,
                                 int64_t need, const char *why) {
  if (leadingDimension < (int64_t)headDimension)
    return fail(MFA_ERR_INVALID_ARGUMENT, std::string("leadingDimension of ") + name + " is smaller than the head dimension");
  return check_stride_multiples(name, leadingDimension, headStride, outer, need, why);
}

mfa_status check_precisions(int precision, int outputPrecision) {
  if (precision != MFA_BF16 && precision != MFA_FP16) return fail(MFA_ERR_INVALID_ARGUMENT, "precision must be MFA_FP16 or MFA_BF16");
  if (outputPrecision != precision && outputPrecision != MFA_FP32)
    return fail(MFA_ERR_INVALID_ARGUMENT, "outputPrecision must be the inputs' 16-bit type or MFA_FP32");
  return MFA_OK;
}

mfa_status check_group(uint32_t heads, uint32_t G) {
  if (heads % G != 0)
    return fail(MFA_ERR_INVALID_ARGUMENT, "heads (" + std::to_string(heads) + ") must be a multiple of headsPerKeyValue (" + std::to_string(G) + ")");
  return MFA_OK;
}

mfa_status check_cache_precision(uint32_t cachePrecision, bool *fp8) {
  if (cachePrecision == MFA_KV_E5M2)
    return fail(MFA_ERR_UNSUPPORTED, "an FP8 KV cache is e4m3 (MFA_KV_E4M3, OCP e4m3fn); e5m2 caches have no kernel");
  *fp8 = cachePrecision == MFA_KV_E4M3;
  return MFA_OK;
}

uint32_t choose_pieces(uint64_t blocks, uint64_t tiles, uint64_t target, uint64_t minTiles, uint64_t maxPieces) {
  if (blocks >= target) return 1;
  uint64_t s = target / blocks;
  if (s > tiles / minTiles) s = tiles / minTiles;
  if (s > maxPieces) s = maxPieces;
  return s < 2 ? 1 : (uint32_t)s;
}

mfa_status check_split_workspace(const void *workspace, uint64_t bytes, uint64_t need, const char *sizeEntry) {
  if (bytes < need)
    return fail(MFA_ERR_INVALID_ARGUMENT, "workspace too small: " + std::to_string(bytes) + " bytes, the launch needs " + std::to_string(need) +
                                              " (" + sizeEntry + ")");
  if ((uintptr_t)workspace % 16 != 0) return fail(MFA_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
  return MFA_OK;
}

mfa_status check_buffers(std::initializer_list<const void *> buffers, const char *names) {
  for (const void *b : buffers)
    if (!b) return fail(MFA_ERR_INVALID_ARGUMENT, "null argument");
  for (const void *b : buffers)
    if ((uintptr_t)b % 16) return fail(MFA_ERR_INVALID_ARGUMENT, std::string(names) + " must be 16-byte aligned");
  return MFA_OK;
}

mfa_status check_float_arrays(std::initializer_list<const void *> arrays, const char *names) {
  for (const void *a : arrays)
    if ((uintptr_t)a % 4) return fail(MFA_ERR_INVALID_ARGUMENT, std::string(names) + " must be 4-byte aligned");
  return MFA_OK;
}

LaunchOptions &LaunchOptions::e4m3(const mfa_kv_quant *block) {
  quant = block;
  if (!block && !refusal) refusal = "null argument", refusalFirst = false;
  return *this;
}

LaunchOptions &LaunchOptions::required_sinks(const mfa_attention_sinks *block) {
  if (!block && !refusal)
    refusal = "null mfa_attention_sinks: the sink entries require the block (mfa_attention_sinks_init; a launch "
              "without sinks: the mfa_window.h entries, or an all-zero block)";
  return optional_sinks(block);
}

LaunchOptions &LaunchOptions::optional_sinks(const mfa_attention_sinks *block) {
  if (block) sinks.tokens = block->sinkTokens, sinks.logits = block->sinkLogits;
  return *this;
}

LaunchOptions &LaunchOptions::ragged_of(const mfa_ragged_rows *block) {
  ragged = block;
  if (!block && !refusal)
    refusal = "null mfa_ragged_rows: the ragged entries require the block (mfa_ragged_rows_init; a padded "
              "launch: the mfa_prefill.h / mfa_window.h / mfa_sink.h entries)";
  return *this;
}

LaunchOptions &LaunchOptions::tree_of(const mfa_attention_tree *block) {
  tree = block;
  if (!block && !refusal)
    refusal = "null mfa_attention_tree: the tree entries require the block (mfa_attention_tree_init; a launch "
              "whose new rows see each other causally: the mfa_sink.h entries)";
  return *this;
}

LaunchOptions &LaunchOptions::split_of(const mfa_key_split *block) {
  split = block;
  if (!block && !refusal)
    refusal = "null mfa_key_split: the split entries require the block (mfa_key_split_init; a launch that is "
              "not cut along the keys: the mfa_prefill.h / mfa_window.h / mfa_sink.h / mfa_tree.h entries, or pieces = 1)";
  return *this;
}

mfa_status entry_check(const LaunchOptions &options, const char *bad) {
  if (options.refusal && (options.refusalFirst || !bad)) return fail(MFA_ERR_INVALID_ARGUMENT, options.refusal);
  return bad ? fail(MFA_ERR_INVALID_ARGUMENT, bad) : MFA_OK;
}

mfa_status check_window_and_sinks(uint32_t window, const Sinks &sinks, bool causal) {
  if (sinks.tokens && !window)
    return fail(MFA_ERR_INVALID_ARGUMENT, "sink tokens need a window: sinkTokens = " + std::to_string(sinks.tokens) +
                                              " keeps the first keys visible under a sliding window, and window is 0 (every key below "
                                              "the frontier is visible already)");
  if (sinks.tokens && !causal)
    return fail(MFA_ERR_INVALID_ARGUMENT, "sink tokens need causal: sinkTokens = " + std::to_string(sinks.tokens) +
                                              " extends a sliding window, which ends at a row's causal frontier");
  if (window && !causal)
    return fail(MFA_ERR_INVALID_ARGUMENT, "a sliding window needs causal: the window is the " + std::to_string(window) +
                                              " keys that end at a row's causal frontier (window 0: no window)");
  return MFA_OK;
}

mfa_status check_softcap(float softcap) {
  if (!(softcap >= 0.0f) || std::isinf(softcap))   // (a NaN fails the comparison)
    return fail(MFA_ERR_INVALID_ARGUMENT, "softcap must be 0 (no cap) or a finite positive number, the cap of cap x tanh(score / cap) in "
                                          "natural-log units (a checkpoint's attn_logit_softcapping), not " + std::to_string(softcap));
  return MFA_OK;
}

mfa_status check_tree(const LaunchOptions &options, bool causal, uint32_t rows, uint32_t rowLimit) {
  const mfa_attention_tree *tree = options.tree;
  if (!tree) return MFA_OK;
  if (!causal)
    return fail(MFA_ERR_INVALID_ARGUMENT, "a speculation tree needs causal: the tree replaces the causal rule among the new rows, which "
                                          "sit behind the cached prefix");
  if (options.window && options.window < rows)
    return fail(MFA_ERR_INVALID_ARGUMENT, "a speculation tree needs a window of at least `rows` keys (or 0: none): window = " +
                                              std::to_string(options.window) + " < rows = " + std::to_string(rows) +
                                              " could leave an ancestor outside a descendant's window");
  if (rowLimit && rows > rowLimit)
    return fail(MFA_ERR_UNSUPPORTED, "a speculation tree holds at most " + std::to_string(rowLimit) +
                                         " nodes, one bit of a uint64 mask each: rows = " + std::to_string(rows));
  if (!tree->masks)
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_attention_tree.masks is required (device array of uint64, [batches][rows], one mask per new row)");
  if ((uintptr_t)tree->masks % 8) return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_attention_tree.masks must be 8-byte aligned");
  if (tree->batchStride < 0 || (tree->batchStride != 0 && (uint64_t)tree->batchStride < rows))
    return fail(MFA_ERR_INVALID_ARGUMENT, "mfa_attention_tree.batchStride must be 0 (one tree shared by every sequence) or at least `rows` elements");
  if (options.softcap != 0.0f)
    return fail(MFA_ERR_UNSUPPORTED, "a soft cap together with a speculation tree has no kernel: softcap must be 0 with a tree");
  if (options.ragged)
    return fail(MFA_ERR_UNSUPPORTED, "a ragged launch together with a speculation tree has no kernel: a tree needs padded rows (queryLengths)");
  return MFA_OK;
}

std::string tree_form(const LaunchOptions &options) {
  if (!options.tree) return std::string();
  return options.tree->batchStride ? ", tree masks per sequence" : ", tree masks shared";
}

} // namespace mfa
