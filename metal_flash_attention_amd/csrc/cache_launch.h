// cache_launch.h -- what the host sides of the launches over a KV cache share (attn_decode16.hip, attn_prefill16.hip,
// kv_cache_append.hip): the checks of paging, operand strides, cache precision and buffer pointers, and of a sliding window and
// attention sinks (Sinks, sinks_of, check_window_and_sinks: decode and prefill) and of a soft cap (check_softcap), each with ONE wording, so that the same mistake is
// refused in the same words whichever launch meets it.  hip_fail, copy_text and time_launches also serve mfa_kernel.hip.  Internal, not part of the ABI.  Every check records its message (fail, mfa_internal.h) and returns the status.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "../../include/mfa_sink.h"
#include "mfa_internal.h"

namespace mfa {

// MFA_ERR_HIP, "<what>: <error name> (<error string>)"
mfa_status hip_fail(hipError_t err, const char *what);

// a launch form's text into the caller's buffer (capacity > 0), cut to fit, always terminated
void copy_text(char *out, size_t capacity, const char *text);

// pageSize 0 is a contiguous cache (*pageShift = 0); otherwise a power of two from 16 to 1024 with a block table, *pageShift its
// logarithm.  `column` != 0: a sequence's row of the table must hold the pages of that many keys (decode, prefill).  0: any positive
// stride (append, whose kernel drops a row whose page lies past the stride).
mfa_status check_paging(uint32_t pageSize, const void *blockTable, int64_t blockTableStride, uint32_t column, uint32_t *pageShift);

// one operand's strides, in elements: leadingDimension, headStride and `outer` (the batch stride, or the page stride of a paged cache)
// are multiples of `need`; `why` ends the message.  check_operand_strides first wants rows of at least headDimension elements.
mfa_status check_stride_multiples(const char *name, int64_t leadingDimension, int64_t headStride, int64_t outer, int64_t need, const char *why);
mfa_status check_operand_strides(const char *name, uint32_t headDimension, int64_t leadingDimension, int64_t headStride, int64_t outer,
                                 int64_t need, const char *why);

// MFA_KV_E5M2 is refused; *fp8 = the cache is MFA_KV_E4M3.  (What else a launch takes, and its words for it, stay with the launch.)
mfa_status check_cache_precision(uint32_t cachePrecision, bool *fp8);

// buffers a kernel reads or writes 16 bytes at a time: all non-null, all 16-byte aligned; `names` as the message lists them
mfa_status check_buffers(std::initializer_list<const void *> buffers, const char *names);
// optional FP32 arrays: null or 4-byte aligned
mfa_status check_float_arrays(std::initializer_list<const void *> arrays, const char *names);

// the sinks of a launch (include/mfa_sink.h): none for the entries of the other headers
struct Sinks {
  uint32_t tokens = 0;
  const float *logits = nullptr;
  bool any() const { return tokens != 0 || logits != nullptr; }
};
// the block of a sink entry, which requires it (null is refused)
mfa_status sinks_of(const mfa_attention_sinks *block, Sinks *sinks);
// sink tokens need a window and causal; a window (0: none) needs causal
mfa_status check_window_and_sinks(uint32_t window, const Sinks &sinks, bool causal);
// the soft cap of a launch (include/mfa_softcap.h): 0 is none, anything but a finite positive number is refused
mfa_status check_softcap(float softcap);

// Times `iterations` calls of run(stream) between two events, after `warmup` untimed ones; nothing more is started after a call that
// failed.  `name` is the kernel a HIP failure is reported under.
template <typename Run>
mfa_status time_launches(hipStream_t stream, int warmup, int iterations, float *milliseconds, const char *name, Run run) {
  hipEvent_t start, stop;
  hipError_t err = hipEventCreate(&start);
  if (err != hipSuccess) return hip_fail(err, "hipEventCreate");
  err = hipEventCreate(&stop);
  if (err != hipSuccess) { (void)hipEventDestroy(start); return hip_fail(err, "hipEventCreate"); }
  for (int i = 0; i < warmup && err == hipSuccess; ++i) err = run(stream);
  if (err == hipSuccess) err = hipEventRecord(start, stream);
  for (int i = 0; i < iterations && err == hipSuccess; ++i) err = run(stream);
  if (err == hipSuccess) err = hipEventRecord(stop, stream);
  if (err == hipSuccess) err = hipEventSynchronize(stop);
  if (err == hipSuccess) err = hipGetLastError();
  if (err == hipSuccess) err = hipEventElapsedTime(milliseconds, start, stop);
  (void)hipEventDestroy(start);
  (void)hipEventDestroy(stop);
  if (err != hipSuccess) return hip_fail(err, name);
  return MFA_OK;
}

} // namespace mfa
